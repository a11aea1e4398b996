"""ctypes binding of the C ABI in include/usn_classify.h (usnetd_amd/libusn.so).

This is thin plumbing for tests, bench.py and the control plane; the product is
the native library.  Loading fails loudly when the library is missing or when
no gfx950 device is present: there is no CPU fallback for the match path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libusn.so")
# the test build (Makefile: the product's device code, a host object that
# reads the A/B and test knobs of the environment); only tests that force
# failures and A/B tools load it -- the product library reads no environment
TEST_LIB_PATH = os.path.join(os.path.dirname(HERE), "build", "test", "libusn.so")

USN_TILE = 1024
USN_WINDOW = 64
USN_WINDOW_MAX = 80
USN_MAX_ENDPOINTS = 4095
USN_MAX_BINS = USN_MAX_ENDPOINTS + 3
USN_ROUND_MAX = 8        # rings of one usn_deliver_round
USN_DELIVER_TILE = 512   # output slots per pack tile of usn_deliver (usn_classify.h)
DV_OVERFLOW, DV_LONG = 1, 2
DV_OVERFLOW_BYTES = 4   # usn_deliver_packed: need_bytes > cap_bytes
DV_DROPPED = 8          # usn_deliver_rings: an offered frame found its ring full
HAS_DELIVER_BRINGS = 1  # USN_HAS_DELIVER_BRINGS: the byte-compact persistent rings (usn_deliver_brings)
DR_MORE = 16            # usn_rings_drain: a ring keeps queued frames after the call
DR_BADCOUNT = 32        # usn_rings_drain: a ring's tail - head exceeds its size (not drained)
DR_BADDESC = 64         # usn_brings_drain: a selected ring's pos16 / lens chain is inconsistent
USN_BDRAIN_UTILE = 4096  # 16-byte units per copy tile of usn_brings_drain (usn_classify.h)
R_WINDOW = 7
PARITY_MASK = 0x00FFFFFF
EP_NIC, EP_HOST, EP_PIPE, EP_UDS = 0, 1, 2, 3
CLS_DROP, CLS_EP, CLS_NIC, CLS_FLOOD = 0, 1, 2, 3
F_CACHE, F_FRAG1, F_FRAGN, F_DHCP, F_HOST, F_LEARN = (1 << 24, 1 << 25, 1 << 26, 1 << 27,
                                                      1 << 28, 1 << 29)
S_STALE, S_STALE_EXTENDS, S_COUT = 1, 2, 8
STATUS = {0: "ok", -22: "EINVAL", -12: "ENOMEM", -17: "EEXIST", -2: "ENOENT", -1: "EPERM",
          -5: "EHIP", -19: "ENODEV", -34: "ERANGE", -16: "EBUSY", -74: "ELIST"}
USN_EBUSY = -16
USN_EINVAL = -22
USN_ERANGE = -34
USN_ENODEV = -19
USN_ELIST = -74


class UsnError(RuntimeError):
    pass


class Want(C.Structure):
    _fields_ = [("dst_addr", C.c_uint32), ("src_addr", C.c_uint32), ("dst_port", C.c_uint16),
                ("src_port", C.c_uint16), ("protocol", C.c_uint8), ("present", C.c_uint8),
                ("_reserved", C.c_uint16)]


class Batch(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("stride", C.c_uint64), ("offsets", C.c_void_p),
                ("lens", C.c_void_p), ("n", C.c_uint64), ("src_endpoint", C.c_uint16),
                ("window", C.c_uint16), ("_reserved", C.c_uint16 * 2)]


# int (*usn_frame_reader)(void *user, uint16_t src, uint64_t index, uint8_t *out, uint32_t cap)
FRAME_READER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint16, C.c_uint64, C.POINTER(C.c_uint8),
                           C.c_uint32)


class Result(C.Structure):
    _fields_ = [("decisions", C.c_void_p), ("index", C.c_void_p), ("bin_off", C.c_void_p),
                ("tiles", C.c_void_p), ("summary", C.c_void_p), ("host_list", C.c_void_p),
                ("scratch", C.c_void_p), ("n", C.c_uint64), ("max_bins", C.c_uint32),
                ("bind_tag", C.c_uint32)]


class FinalizeInfo(C.Structure):
    _fields_ = [("n_host", C.c_uint32), ("n_patched", C.c_uint32), ("n_learned", C.c_uint32),
                ("flags", C.c_uint32), ("class_count", C.c_uint32 * 4)]


class DeliveryHdr(C.Structure):
    _fields_ = [("need", C.c_uint32), ("cap", C.c_uint32), ("flags", C.c_uint32),
                ("n_recv", C.c_uint32)]


class Delivery(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("lens", C.c_void_p), ("src", C.c_void_p),
                ("ep_off", C.c_void_p), ("hdr", C.c_void_p), ("cap", C.c_uint64),
                ("slot", C.c_uint32), ("_r", C.c_uint32)]


class RDelivery(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("lens", C.c_void_p), ("src", C.c_void_p),
                ("ep_off", C.c_void_p), ("seg_off", C.c_void_p), ("hdr", C.c_void_p),
                ("cap", C.c_uint64), ("slot", C.c_uint32), ("_r", C.c_uint32)]


class PDeliveryHdr(C.Structure):
    _fields_ = [("need", C.c_uint32), ("cap", C.c_uint32), ("flags", C.c_uint32),
                ("n_recv", C.c_uint32), ("need_bytes", C.c_uint64), ("cap_bytes", C.c_uint64)]


class PDelivery(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("off16", C.c_void_p), ("lens", C.c_void_p),
                ("src", C.c_void_p), ("ep_off", C.c_void_p), ("ep_boff", C.c_void_p),
                ("hdr", C.c_void_p), ("cap", C.c_uint64), ("cap_bytes", C.c_uint64)]


class RingSetHdr(C.Structure):
    _fields_ = [("offered", C.c_uint64), ("dropped", C.c_uint64), ("accepted", C.c_uint32),
                ("n_recv", C.c_uint32), ("flags", C.c_uint32), ("_r", C.c_uint32)]


class RingSet(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("lens", C.c_void_p), ("src", C.c_void_p),
                ("ring_off", C.c_void_p), ("head", C.c_void_p), ("tail", C.c_void_p),
                ("first", C.c_void_p), ("acc", C.c_void_p), ("drop", C.c_void_p),
                ("seg_acc", C.c_void_p), ("hdr", C.c_void_p), ("total", C.c_uint64),
                ("slot", C.c_uint32), ("ready", C.c_uint32)]


class BRingSetHdr(C.Structure):
    _fields_ = [("offered", C.c_uint64), ("dropped", C.c_uint64), ("accepted_units", C.c_uint64),
                ("accepted", C.c_uint32), ("n_recv", C.c_uint32), ("flags", C.c_uint32),
                ("_r", C.c_uint32)]


class BRingSet(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("frames", "lens", "src", "pos16", "desc_off", "unit_off",
                                          "head", "tail", "btail", "first", "bfirst", "acc", "drop",
                                          "acc_units", "seg_acc", "hdr")] + \
               [("total_desc", C.c_uint64), ("total_units", C.c_uint64), ("ready", C.c_uint32),
                ("_r", C.c_uint32)]


class DrainHdr(C.Structure):
    _fields_ = [("need_bytes", C.c_uint64), ("cap_bytes", C.c_uint64), ("selected", C.c_uint32),
                ("taken", C.c_uint32), ("n_recv", C.c_uint32), ("flags", C.c_uint32)]


class Drain(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("off16", C.c_void_p), ("lens", C.c_void_p),
                ("src", C.c_void_p), ("ep_off", C.c_void_p), ("ep_boff", C.c_void_p),
                ("budget", C.c_void_p), ("from_", C.c_void_p), ("take", C.c_void_p),
                ("left", C.c_void_p), ("hdr", C.c_void_p), ("cap", C.c_uint64),
                ("cap_bytes", C.c_uint64)]


TILE_HDR_DTYPE = np.dtype([("n_frames", "<u2"), ("_r0", "<u2"), ("n_host", "<u2"),
                           ("bin_nic", "<u2"), ("class_count", "<u2", (4,)), ("last_state", "<u4"),
                           ("last_dst", "<u4"), ("last_idx", "<u4"), ("last_info", "<u4", (4,)),
                           ("_pad", "<u4")])
SUMMARY_DTYPE = np.dtype([("flags", "<u4"), ("first_break", "<u4"), ("n_frames", "<u4"),
                          ("n_tiles", "<u4"), ("cin_state", "<u4"), ("cin_dst", "<u4"),
                          ("cin_info", "<u4", (4,)), ("cout_state", "<u4"), ("cout_dst", "<u4"),
                          ("cout_info", "<u4", (4,)), ("n_ep", "<u4"), ("n_bins", "<u4"),
                          ("host_epoch", "<u4"), ("_pad", "<u4")])
RULE_DTYPE = np.dtype([("dst_addr", "<u4"), ("src_addr", "<u4"), ("dst_port", "<u2"),
                       ("src_port", "<u2"), ("protocol", "u1"), ("present", "u1"),
                       ("endpoint", "<u2")])
assert TILE_HDR_DTYPE.itemsize == 48 and SUMMARY_DTYPE.itemsize == 80 and RULE_DTYPE.itemsize == 16

_libs: dict = {}


def load(path: str | None = None):
    """Load libusn.so (raises if it was not built).  `path` selects another
    build of the same ABI (A/B experiments in tools/)."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise UsnError("%s is missing: run `make` (or __graft_entry__.build()) first; "
                       "the match path has no CPU fallback" % path)
    L = C.CDLL(path)
    P, I, U16, U32, U64, SZ = C.c_void_p, C.c_int, C.c_uint16, C.c_uint32, C.c_uint64, C.c_size_t
    sig = {
        "usn_abi_version": ([], I), "usn_strerror": ([I], C.c_char_p),
        "usn_last_hip_error": ([], I),
        "usn_ctx_create": ([I, C.POINTER(P)], I), "usn_ctx_destroy": ([P], None),
        "usn_endpoint_add": ([P, U16, I, C.c_int32], I), "usn_endpoint_remove": ([P, U16], I),
        "usn_add_match": ([P, C.POINTER(Want), U16, I], I),
        "usn_remove_match": ([P, C.POINTER(Want), U16], I),
        "usn_rule_count": ([P], I),
        "usn_rules_get": ([P, P, P, P, U32], I),
        "usn_lookup": ([P, C.POINTER(Want)], I),
        "usn_bridge_add": ([P, C.c_char_p], I), "usn_bridge_count": ([P], I),
        "usn_bridge_set": ([P, P, U32], I), "usn_table_build": ([P, P, U32], I),
        "usn_frag_clear": ([P], I), "usn_cache_clear": ([P, U16], I),
        "usn_result_bytes": ([U64], SZ), "usn_result_bytes_ep": ([U64, U32], SZ),
        "usn_result_bind": ([P, SZ, U64, C.POINTER(Result)], I),
        "usn_result_release": ([P, C.POINTER(Result)], I),
        "usn_classify": ([P, C.POINTER(Batch), C.POINTER(Result), P], I),
        "usn_finalize": ([P, C.POINTER(Batch), C.POINTER(Result), P, C.POINTER(FinalizeInfo)], I),
        "usn_dev_alloc": ([P, SZ, C.POINTER(P)], I), "usn_dev_free": ([P, P], I),
        "usn_host_alloc_pinned": ([P, SZ, C.POINTER(P)], I), "usn_host_free_pinned": ([P, P], I),
        "usn_memcpy_h2d": ([P, P, P, SZ, P], I), "usn_memcpy_d2h": ([P, P, P, SZ, P], I),
        "usn_memset_d": ([P, P, I, SZ, P], I),
        "usn_stream_create": ([P, C.POINTER(P)], I), "usn_stream_destroy": ([P, P], I),
        "usn_stream_sync": ([P, P], I), "usn_device_sync": ([P], I),
        "usn_event_create": ([P, C.POINTER(P)], I), "usn_event_destroy": ([P, P], I),
        "usn_event_record": ([P, P, P], I),
        "usn_event_elapsed_ms": ([P, P, P, C.POINTER(C.c_float)], I),
        "usn_stream_wait_event": ([P, P, P], I),
        "usn_classify_multi": ([P, P, P, U32, P], I),
        "usn_set_frame_reader": ([P, FRAME_READER, P], I),
        "usn_ctx_create_group": ([P, U32, C.POINTER(P)], I),
        "usn_ctx_replicas": ([P], I), "usn_replica_select": ([P, U32], I),
        "usn_replica_device": ([P, U32], I),
        "usn_set_lists_async": ([P, I], I), "usn_lists_wait": ([P, C.POINTER(Result), P], I),
        "usn_delivery_bytes": ([U64, U32], SZ),
        "usn_delivery_bind": ([P, SZ, U64, U32, C.POINTER(Delivery)], I),
        "usn_deliver": ([P, C.POINTER(Batch), C.POINTER(Result), C.POINTER(Delivery), P], I),
        "usn_deliver_info": ([P, C.POINTER(Delivery), P, C.POINTER(DeliveryHdr)], I),
        "usn_pdelivery_bytes": ([U64, U64], SZ),
        "usn_pdelivery_bind": ([P, SZ, U64, U64, C.POINTER(PDelivery)], I),
        "usn_deliver_packed": ([P, C.POINTER(Batch), C.POINTER(Result), C.POINTER(PDelivery), P], I),
        "usn_deliver_packed_info": ([P, C.POINTER(PDelivery), P, C.POINTER(PDeliveryHdr)], I),
        "usn_rdelivery_bytes": ([U64, U32], SZ),
        "usn_rdelivery_bind": ([P, SZ, U64, U32, C.POINTER(RDelivery)], I),
        "usn_deliver_round": ([P, P, P, U32, C.POINTER(RDelivery), P], I),
        "usn_deliver_round_info": ([P, C.POINTER(RDelivery), P, C.POINTER(DeliveryHdr)], I),
        "usn_ringset_bytes": ([U64, U32], SZ),
        "usn_ringset_bind": ([P, SZ, U64, U32, C.POINTER(RingSet)], I),
        "usn_ringset_init": ([P, C.POINTER(RingSet), P, U32, P], I),
        "usn_ringset_set_head": ([P, C.POINTER(RingSet), P, U32, P], I),
        "usn_deliver_rings": ([P, P, P, U32, C.POINTER(RingSet), P], I),
        "usn_deliver_rings_info": ([P, C.POINTER(RingSet), P, C.POINTER(RingSetHdr)], I),
        "usn_drain_bytes": ([U64, U64], SZ),
        "usn_drain_bind": ([P, SZ, U64, U64, C.POINTER(Drain)], I),
        "usn_drain_set_budget": ([P, C.POINTER(Drain), P, U32, P], I),
        "usn_rings_drain": ([P, C.POINTER(RingSet), C.POINTER(Drain), P], I),
        "usn_rings_drain_info": ([P, C.POINTER(Drain), P, C.POINTER(DrainHdr)], I),
        "usn_bringset_bytes": ([U64, U64], SZ),
        "usn_bringset_bind": ([P, SZ, U64, U64, C.POINTER(BRingSet)], I),
        "usn_bringset_init": ([P, C.POINTER(BRingSet), P, P, U32, P], I),
        "usn_bringset_set_head": ([P, C.POINTER(BRingSet), P, U32, P], I),
        "usn_deliver_brings": ([P, P, P, U32, C.POINTER(BRingSet), P], I),
        "usn_deliver_brings_info": ([P, C.POINTER(BRingSet), P, C.POINTER(BRingSetHdr)], I),
        "usn_brings_drain": ([P, C.POINTER(BRingSet), C.POINTER(Drain), P], I),
        "usn_brings_drain_info": ([P, C.POINTER(Drain), P, C.POINTER(DrainHdr)], I),
    }
    optional = {"usn_set_frame_reader", "usn_ctx_create_group", "usn_ctx_replicas",
                "usn_replica_select", "usn_replica_device", "usn_result_bytes_ep",
                "usn_set_lists_async", "usn_lists_wait", "usn_result_release", "usn_delivery_bytes",
                "usn_delivery_bind", "usn_deliver", "usn_deliver_info", "usn_pdelivery_bytes",
                "usn_pdelivery_bind", "usn_deliver_packed", "usn_deliver_packed_info",
                "usn_rdelivery_bytes", "usn_rdelivery_bind", "usn_deliver_round",
                "usn_deliver_round_info", "usn_ringset_bytes", "usn_ringset_bind", "usn_ringset_init",
                "usn_ringset_set_head", "usn_deliver_rings",
                "usn_deliver_rings_info", "usn_drain_bytes", "usn_drain_bind", "usn_drain_set_budget",
                "usn_rings_drain", "usn_rings_drain_info", "usn_bringset_bytes", "usn_bringset_bind",
                "usn_bringset_init", "usn_bringset_set_head", "usn_deliver_brings",
                "usn_deliver_brings_info", "usn_brings_drain", "usn_brings_drain_info"}   # A/B builds of older ABI versions lack these
    for name, (args, res) in sig.items():
        if name in optional and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _libs[path] = L
    return L


EXPORTED = ["usn_abi_version", "usn_strerror", "usn_last_hip_error", "usn_ctx_create",
            "usn_ctx_destroy", "usn_endpoint_add", "usn_endpoint_remove", "usn_add_match",
            "usn_remove_match", "usn_rule_count", "usn_rules_get", "usn_lookup", "usn_bridge_add",
            "usn_bridge_count", "usn_frag_clear", "usn_cache_clear", "usn_result_bytes", "usn_result_bytes_ep",
            "usn_result_bind", "usn_classify", "usn_finalize", "usn_dev_alloc", "usn_dev_free",
            "usn_host_alloc_pinned", "usn_host_free_pinned", "usn_memcpy_h2d", "usn_memcpy_d2h",
            "usn_memset_d", "usn_stream_create", "usn_stream_destroy", "usn_stream_sync",
            "usn_device_sync", "usn_event_create", "usn_event_destroy", "usn_event_record",
            "usn_event_elapsed_ms", "usn_stream_wait_event", "usn_classify_multi",
            "usn_bridge_set", "usn_table_build", "usn_set_frame_reader", "usn_ctx_create_group",
            "usn_ctx_replicas", "usn_replica_select", "usn_replica_device", "usn_set_lists_async",
            "usn_lists_wait", "usn_result_release", "usn_delivery_bytes", "usn_delivery_bind",
            "usn_deliver", "usn_deliver_info", "usn_pdelivery_bytes", "usn_pdelivery_bind",
            "usn_deliver_packed", "usn_deliver_packed_info", "usn_rdelivery_bytes",
            "usn_rdelivery_bind", "usn_deliver_round", "usn_deliver_round_info",
            "usn_ringset_bytes", "usn_ringset_bind", "usn_ringset_init", "usn_ringset_set_head",
            "usn_deliver_rings", "usn_deliver_rings_info", "usn_drain_bytes", "usn_drain_bind",
            "usn_drain_set_budget", "usn_rings_drain", "usn_rings_drain_info", "usn_bringset_bytes",
            "usn_bringset_bind", "usn_bringset_init", "usn_bringset_set_head", "usn_deliver_brings",
            "usn_deliver_brings_info", "usn_brings_drain", "usn_brings_drain_info"]


def check(rc, what=""):
    if rc < 0:
        L = load() if LIB_PATH in _libs or not _libs else next(iter(_libs.values()))
        extra = ""
        if rc == -5:
            extra = " (hipError %d)" % L.usn_last_hip_error()
        raise UsnError("%s failed: %s%s" % (what, STATUS.get(rc, rc), extra))
    return rc


def ip2int(s):
    if s is None:
        return None
    if isinstance(s, int):
        return s
    a, b, c, d = (int(x) for x in s.split("."))
    return (a << 24) | (b << 16) | (c << 8) | d


def make_want(dst, proto, dport=None, src=None, sport=None) -> Want:
    w = Want()
    w.dst_addr = ip2int(dst)
    w.protocol = proto
    p = 0
    if dport is not None:
        p |= 1
        w.dst_port = dport
    if src is not None:
        p |= 2
        w.src_addr = ip2int(src)
    if sport is not None:
        p |= 4
        w.src_port = sport
    w.present = p
    return w


def want_from_dict(d) -> Want:
    return make_want(d["dst"], d["proto"], d.get("dport"), d.get("src"), d.get("sport"))


class DevBuf:
    """A device allocation owned by a Ctx."""

    def __init__(self, ctx: "Ctx", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(ctx.L.usn_dev_alloc(ctx.h, max(self.nbytes, 16), C.byref(p)), "usn_dev_alloc")
        self.ptr = p.value

    def free(self):
        if self.ptr:
            self.ctx.L.usn_dev_free(self.ctx.h, self.ptr)
            self.ptr = None

    def upload(self, arr: np.ndarray, stream=None, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        check(self.ctx.L.usn_memcpy_h2d(self.ctx.h, self.ptr + offset, arr.ctypes.data,
                                        arr.nbytes, stream), "h2d")
        if stream is None:
            self.ctx.sync()

    def download(self, dtype, count, offset=0, stream=None) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        check(self.ctx.L.usn_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr + offset,
                                        out.nbytes, stream), "d2h")
        self.ctx.sync(stream)
        return out


class Ctx:
    """One usn_ctx bound to one gfx950 device (the daemon's match state)."""

    def __init__(self, device: int = 0, libpath: str | None = None, devices=None):
        """devices: a list of HIP devices -> one registry with a device
        replica per entry (usn_ctx_create_group); replica 0 is selected."""
        self.L = load(libpath)
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            check(self.L.usn_ctx_create_group(C.cast(arr, C.c_void_p), len(devices), C.byref(h)),
                  "usn_ctx_create_group")
            device = devices[0]
        else:
            check(self.L.usn_ctx_create(device, C.byref(h)), "usn_ctx_create")
        self.h = h.value
        self.device = device

    def replicas(self) -> int:
        return check(self.L.usn_ctx_replicas(self.h), "usn_ctx_replicas")

    def select(self, replica: int):
        """Classify and device plumbing act on this replica from now on."""
        check(self.L.usn_replica_select(self.h, replica), "usn_replica_select")
        self.device = check(self.L.usn_replica_device(self.h, replica), "usn_replica_device")

    def close(self):
        if self.h:
            self.L.usn_ctx_destroy(self.h)
            self.h = None

    # --- control plane --------------------------------------------------------
    def endpoint_add(self, eid, kind, for_nic=None):
        return check(self.L.usn_endpoint_add(self.h, eid, kind, -1 if for_nic is None else for_nic),
                     "usn_endpoint_add")

    def endpoint_remove(self, eid):
        return check(self.L.usn_endpoint_remove(self.h, eid), "usn_endpoint_remove")

    def add_match(self, want: Want, owner: int, sticky=False) -> int:
        rc = self.L.usn_add_match(self.h, C.byref(want), owner, int(bool(sticky)))
        return rc if rc in (0, 1) else check(rc, "usn_add_match")

    def remove_match(self, want: Want, requester: int) -> int:
        rc = self.L.usn_remove_match(self.h, C.byref(want), requester)
        return -1 if rc == -1 else check(rc, "usn_remove_match")

    def rule_count(self):
        return check(self.L.usn_rule_count(self.h), "usn_rule_count")

    def rules(self):
        n = self.rule_count()
        ws = (Want * max(n, 1))()
        owners = np.zeros(max(n, 1), np.uint16)
        sticky = np.zeros(max(n, 1), np.uint8)
        got = check(self.L.usn_rules_get(self.h, C.cast(ws, C.c_void_p), owners.ctypes.data,
                                         sticky.ctypes.data, n), "usn_rules_get")
        return [(ws[i], int(owners[i]), bool(sticky[i])) for i in range(got)]

    def lookup(self, want: Want) -> int:
        rc = self.L.usn_lookup(self.h, C.byref(want))
        return -1 if rc == -2 else check(rc, "usn_lookup")

    def bridge_add(self, mac: bytes):
        check(self.L.usn_bridge_add(self.h, bytes(mac)), "usn_bridge_add")

    def table_build(self, rules) -> int:
        """rules: [(Want, owner, sticky)] -> usn_table_build (bulk replace)."""
        arr = np.zeros(len(rules), RULE_DTYPE)
        for i, (w, owner, sticky) in enumerate(rules):
            arr[i] = (w.dst_addr, w.src_addr, w.dst_port, w.src_port, w.protocol,
                      (w.present & 7) | (0x80 if sticky else 0), owner)
        return check(self.L.usn_table_build(self.h, arr.ctypes.data, len(rules)),
                     "usn_table_build")

    def bridge_set(self, macs) -> None:
        arr = np.frombuffer(b"".join(bytes(m) for m in macs), np.uint8) if macs else np.zeros(6, np.uint8)
        check(self.L.usn_bridge_set(self.h, arr.ctypes.data, len(macs)), "usn_bridge_set")

    def bridge_count(self) -> int:
        return check(self.L.usn_bridge_count(self.h), "usn_bridge_count")

    def frag_clear(self):
        check(self.L.usn_frag_clear(self.h), "usn_frag_clear")

    def cache_clear(self, eid):
        check(self.L.usn_cache_clear(self.h, eid), "usn_cache_clear")

    def set_frame_reader(self, fn):
        """fn(src_endpoint, index) -> bytes of that frame of the batch being
        finalized (the host copy, whole or its first USN_WINDOW_MAX bytes);
        None unregisters.  The ctypes callback is kept alive on the Ctx."""
        if fn is None:
            self._reader = None
            check(self.L.usn_set_frame_reader(self.h, FRAME_READER(), None), "usn_set_frame_reader")
            return

        def cb(user, src, index, out, cap):
            try:
                data = bytes(fn(int(src), int(index)))[:cap]
            except Exception:
                return -1
            C.memmove(out, data, len(data))
            return len(data)
        self._reader = FRAME_READER(cb)
        check(self.L.usn_set_frame_reader(self.h, self._reader, None), "usn_set_frame_reader")

    # --- plumbing ---------------------------------------------------------------
    def alloc(self, nbytes) -> DevBuf:
        return DevBuf(self, nbytes)

    def sync(self, stream=None):
        if stream is None:
            check(self.L.usn_device_sync(self.h), "usn_device_sync")
        else:
            check(self.L.usn_stream_sync(self.h, stream), "usn_stream_sync")

    def stream(self):
        s = C.c_void_p()
        check(self.L.usn_stream_create(self.h, C.byref(s)), "usn_stream_create")
        return s.value

    def event(self):
        e = C.c_void_p()
        check(self.L.usn_event_create(self.h, C.byref(e)), "usn_event_create")
        return e.value

    def record(self, ev, stream):
        check(self.L.usn_event_record(self.h, ev, stream), "usn_event_record")

    def wait_event(self, stream, ev):
        check(self.L.usn_stream_wait_event(self.h, stream, ev), "usn_stream_wait_event")

    def elapsed_ms(self, a, b) -> float:
        ms = C.c_float()
        check(self.L.usn_event_elapsed_ms(self.h, a, b, C.byref(ms)), "usn_event_elapsed_ms")
        return ms.value

    # --- hot path -----------------------------------------------------------------
    def classify(self, batch: "DeviceBatch", result: "DeviceResult", stream=None):
        check(self.L.usn_classify(self.h, C.byref(batch.desc), C.byref(result.desc), stream),
              "usn_classify")

    def classify_multi(self, batches, results, stream=None):
        """One launch over several batches (usn_classify_multi): rx rings of
        distinct NIC sources, or up to eight consecutive rings of a sending
        endpoint (in one tx grid)."""
        n = len(batches)
        ba = (Batch * n)(*[b.desc for b in batches])
        ra = (Result * n)(*[r.desc for r in results])
        check(self.L.usn_classify_multi(self.h, C.cast(ba, C.c_void_p), C.cast(ra, C.c_void_p), n,
                                        stream), "usn_classify_multi")

    def set_lists_async(self, on=True):
        """Build the per-endpoint lists on a side stream (usn_set_lists_async)."""
        check(self.L.usn_set_lists_async(self.h, int(bool(on))), "usn_set_lists_async")

    def scatter_fallbacks(self) -> int:
        """Scatter chunks (on this replica's device, since the library was
        loaded) whose optimistic ranks were not stably sorted and were ranked
        again the ballot way (expected 0; usn_debug_scatter_fallbacks)."""
        f = self.L.usn_debug_scatter_fallbacks
        f.argtypes = [C.c_void_p]
        f.restype = C.c_int64
        return check(f(self.h), "usn_debug_scatter_fallbacks")

    def lists_wait(self, result: "DeviceResult", stream=None):
        check(self.L.usn_lists_wait(self.h, C.byref(result.desc), stream), "usn_lists_wait")

    def finalize(self, batch: "DeviceBatch", result: "DeviceResult", stream=None) -> FinalizeInfo:
        info = FinalizeInfo()
        check(self.L.usn_finalize(self.h, C.byref(batch.desc), C.byref(result.desc), stream,
                                  C.byref(info)), "usn_finalize")
        return info

    def deliver(self, batch: "DeviceBatch", result: "DeviceResult", delivery: "DeviceDelivery",
                stream=None):
        """Pack every receiver's output ring of a classified batch on the device
        (usn_deliver): asynchronous on `stream`; after finalize() for a batch that
        needs the host stage."""
        check(self.L.usn_deliver(self.h, C.byref(batch.desc), C.byref(result.desc),
                                 C.byref(delivery.desc), stream), "usn_deliver")

    def deliver_packed(self, batch: "DeviceBatch", result: "DeviceResult",
                       delivery: "DevicePackedDelivery", stream=None):
        """deliver() with byte-compact rings (usn_deliver_packed): every frame
        behind the one before it, padded to 16 bytes."""
        check(self.L.usn_deliver_packed(self.h, C.byref(batch.desc), C.byref(result.desc),
                                        C.byref(delivery.desc), stream), "usn_deliver_packed")

    def deliver_round(self, batches, results, delivery: "DeviceRoundDelivery", stream=None):
        """One ring per endpoint for a whole poll round (usn_deliver_round): the
        up to USN_ROUND_MAX rings in poll order, every result final; endpoint e's
        ring is its usn_deliver segments of ring 0, 1, ... back to back."""
        n = len(batches)
        ba = (Batch * n)(*[b.desc for b in batches])
        ra = (Result * n)(*[r.desc for r in results])
        check(self.L.usn_deliver_round(self.h, C.cast(ba, C.c_void_p), C.cast(ra, C.c_void_p), n,
                                       C.byref(delivery.desc), stream), "usn_deliver_round")

    def deliver_rings(self, batches, results, rs: "DeviceRingSet", stream=None):
        """Append a poll round to the persistent endpoint rings of `rs`
        (usn_deliver_rings): deliver_round's rings and order; each receiver takes
        what its ring has room for and drops the rest, tails move last."""
        n = len(batches)
        ba = (Batch * n)(*[b.desc for b in batches])
        ra = (Result * n)(*[r.desc for r in results])
        check(self.L.usn_deliver_rings(self.h, C.cast(ba, C.c_void_p), C.cast(ra, C.c_void_p), n,
                                       C.byref(rs.desc), stream), "usn_deliver_rings")

    def deliver_brings(self, batches, results, rs: "DeviceBRingSet", stream=None):
        """Append a poll round to the persistent byte-compact rings of `rs`
        (usn_deliver_brings): deliver_rings' round and order; a receiver takes
        frames while a descriptor and the frame's 16-byte units are free and
        drops the rest of its round, tail and btail move last."""
        n = len(batches)
        ba = (Batch * n)(*[b.desc for b in batches])
        ra = (Result * n)(*[r.desc for r in results])
        check(self.L.usn_deliver_brings(self.h, C.cast(ba, C.c_void_p), C.cast(ra, C.c_void_p), n,
                                        C.byref(rs.desc), stream), "usn_deliver_brings")

    def drain_brings(self, rs: "DeviceBRingSet", dr: "DeviceDrain", stream=None):
        """Take up to dr's budgets of the oldest queued frames out of every byte ring
        of `rs`, their units back to back in `dr`, and move the heads
        (usn_brings_drain): three launches, no copy."""
        check(self.L.usn_brings_drain(self.h, C.byref(rs.desc), C.byref(dr.desc), stream), "usn_brings_drain")

    def drain_rings(self, rs: "DeviceRingSet", dr: "DeviceDrain", stream=None):
        """Take up to dr's budgets of the oldest queued frames of every ring of
        `rs`, byte-compact into `dr`, and move the heads (usn_rings_drain):
        asynchronous on `stream`, which must also order the appends to `rs`."""
        check(self.L.usn_rings_drain(self.h, C.byref(rs.desc), C.byref(dr.desc), stream), "usn_rings_drain")


class DeviceBatch:
    """Frames + lengths resident in HBM (one drained rx ring)."""

    def __init__(self, ctx: Ctx, frames: np.ndarray, lens: np.ndarray, src: int,
                 stride: int = 0, offsets: np.ndarray | None = None, pad: int = USN_WINDOW,
                 window: int | None = None):
        """window: readable bytes of each frame at its start (usn_batch.window);
        default min(stride, 2048) for strided layouts, USN_WINDOW for offsets."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        self.n = int(lens.shape[0])
        self.buf = ctx.alloc(frames.nbytes + pad)
        self.buf.upload(frames)
        self.lbuf = ctx.alloc(lens.nbytes)
        self.lbuf.upload(lens)
        self.obuf = None
        self.desc = Batch()
        self.desc.frames = self.buf.ptr
        self.desc.lens = self.lbuf.ptr
        self.desc.n = self.n
        self.desc.src_endpoint = src
        if window is None:
            window = min(int(stride), 2048) if offsets is None and stride else USN_WINDOW
        self.desc.window = window
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            self.obuf = ctx.alloc(offsets.nbytes)
            self.obuf.upload(offsets)
            self.desc.offsets = self.obuf.ptr
            self.desc.stride = 0
        else:
            self.desc.stride = stride

    def set_src(self, src):
        self.desc.src_endpoint = src

    def free(self):
        for b in (self.buf, self.lbuf, self.obuf):
            if b is not None:
                b.free()


class DeviceResult:
    """One usn_result: decisions, the per-endpoint lists (index, bin_off),
    tile headers, summary.  max_endpoints sizes the scatter scratch for
    endpoint ids below it (default: any id, USN_MAX_ENDPOINTS)."""

    def __init__(self, ctx: Ctx, n: int, max_endpoints: int | None = None):
        self.ctx = ctx
        self.n = int(n)
        if max_endpoints is None:
            nbytes = ctx.L.usn_result_bytes(self.n)
        else:
            nbytes = ctx.L.usn_result_bytes_ep(self.n, int(max_endpoints))
        self.buf = ctx.alloc(nbytes)
        self.desc = Result()
        check(ctx.L.usn_result_bind(self.buf.ptr, nbytes, self.n, C.byref(self.desc)),
              "usn_result_bind")
        self.ntiles = (self.n + USN_TILE - 1) // USN_TILE

    def _off(self, ptr):
        return ptr - self.buf.ptr

    def decisions(self, n=None) -> np.ndarray:
        return self.buf.download(np.uint32, n or self.n, self._off(self.desc.decisions))

    def index(self, n=None) -> np.ndarray:
        return self.buf.download(np.uint32, n or self.n, self._off(self.desc.index))

    def bin_off(self, nbins=None) -> np.ndarray:
        nb = int(self.summary()["n_bins"]) if nbins is None else nbins
        return self.buf.download(np.uint32, nb + 1, self._off(self.desc.bin_off))

    def lists(self, n=None) -> dict:
        """{bin: frame indices in frame order} of the device-wide scatter
        (bins: endpoint ids, then n_ep = NIC, n_ep + 1 = FLOOD, n_ep + 2 = DROP)."""
        off = self.bin_off()
        idx = self.index(n)
        return {b: idx[off[b]:off[b + 1]] for b in range(off.size - 1) if off[b + 1] > off[b]}

    def tiles(self) -> np.ndarray:
        raw = self.buf.download(np.uint8, self.ntiles * TILE_HDR_DTYPE.itemsize,
                                self._off(self.desc.tiles))
        return raw.view(TILE_HDR_DTYPE)

    def summary(self) -> np.ndarray:
        raw = self.buf.download(np.uint8, SUMMARY_DTYPE.itemsize, self._off(self.desc.summary))
        return raw.view(SUMMARY_DTYPE)[0]

    def free(self):
        """usn_result_release (the context's records of this result), then the memory"""
        if self.buf is None:
            return
        if hasattr(self.ctx.L, "usn_result_release") and self.ctx.h:
            check(self.ctx.L.usn_result_release(self.ctx.h, C.byref(self.desc)), "usn_result_release")
        self.buf.free()
        self.buf = None


def dec_bin(dec: np.ndarray, n_ep: int) -> np.ndarray:
    """bin of each decision word: its endpoint id (class EP), else NIC / FLOOD / DROP after the
    endpoints (usn_classify.h, usn_result.index)."""
    cls = (dec >> 16) & 0xF
    ep = dec & 0xFFFF
    other = n_ep + ((cls + 2) & 3)
    return np.where(cls == CLS_EP, ep, other).astype(np.int64)


def expected_lists(dec: np.ndarray, n_ep: int) -> dict:
    """{bin: frame indices} a stable scatter of these decisions must produce."""
    bins = dec_bin(np.asarray(dec, np.uint32), n_ep)
    order = np.argsort(bins, kind="stable")
    sb = bins[order]
    cuts = np.flatnonzero(np.diff(sb)) + 1
    return {int(sb[g[0]]): order[g].astype(np.uint32) for g in np.split(np.arange(sb.size), cuts)
            if g.size}


class DeviceDelivery:
    """One usn_delivery: cap_slots output slots of `slot` bytes, their lens[] and
    src[], the per-endpoint slot offsets and the header.  `poison` fills the
    whole allocation first (tests: what the kernels did not write stays)."""

    def __init__(self, ctx: Ctx, cap_slots: int, slot: int, poison: int | None = None):
        self.ctx = ctx
        self.cap = int(cap_slots)
        self.slot = int(slot)
        nbytes = ctx.L.usn_delivery_bytes(self.cap, self.slot)
        if nbytes == 0:
            raise UsnError("usn_delivery_bytes: bad capacity %d or slot %d" % (self.cap, self.slot))
        self.buf = ctx.alloc(nbytes)
        self.desc = Delivery()
        check(ctx.L.usn_delivery_bind(self.buf.ptr, nbytes, self.cap, self.slot, C.byref(self.desc)),
              "usn_delivery_bind")
        if poison is not None:
            check(ctx.L.usn_memset_d(ctx.h, self.buf.ptr, poison, nbytes, None), "usn_memset_d")
            ctx.sync()

    def info(self, stream=None, strict=True) -> DeliveryHdr:
        """The header after the delivery on `stream` finished.  strict: raise on
        USN_DV_OVERFLOW / USN_DV_LONG (USN_ERANGE); else return it with .status."""
        h = DeliveryHdr()
        rc = self.ctx.L.usn_deliver_info(self.ctx.h, C.byref(self.desc), stream, C.byref(h))
        if strict or rc != USN_ERANGE:
            check(rc, "usn_deliver_info")
        h.status = rc
        return h

    def _get(self, ptr, dtype, count):
        if count == 0:
            return np.empty(0, dtype)
        return self.buf.download(dtype, count, ptr - self.buf.ptr)

    def ep_off(self) -> np.ndarray:
        """ring of endpoint e = slots [ep_off[e], ep_off[e + 1])"""
        return self._get(self.desc.ep_off, np.uint32, USN_MAX_ENDPOINTS + 1)

    def lens(self, k0=0, k1=None) -> np.ndarray:
        k1 = self.cap if k1 is None else k1
        return self._get(self.desc.lens + 2 * k0, np.uint16, k1 - k0)

    def src(self, k0=0, k1=None) -> np.ndarray:
        k1 = self.cap if k1 is None else k1
        return self._get(self.desc.src + 4 * k0, np.uint32, k1 - k0)

    def slots(self, k0=0, k1=None) -> np.ndarray:
        k1 = self.cap if k1 is None else k1
        return self._get(self.desc.frames + self.slot * k0, np.uint8,
                         (k1 - k0) * self.slot).reshape(k1 - k0, self.slot)

    def ring(self, e: int):
        """(src_idx, lens, bytes[k, slot]) of endpoint e's ring"""
        off = self.ep_off()
        k0, k1 = int(off[e]), int(off[e + 1])
        return self.src(k0, k1), self.lens(k0, k1), self.slots(k0, k1)

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None


class DeviceRoundDelivery(DeviceDelivery):
    """One usn_rdelivery: DeviceDelivery's arrays for a poll round, plus seg_off:
    segment (e, k), ring k's frames for endpoint e, is slots
    [seg_off[8e + k], seg_off[8e + k + 1])."""

    def __init__(self, ctx: Ctx, cap_slots: int, slot: int, poison: int | None = None):
        self.ctx = ctx
        self.cap = int(cap_slots)
        self.slot = int(slot)
        nbytes = ctx.L.usn_rdelivery_bytes(self.cap, self.slot)
        if nbytes == 0:
            raise UsnError("usn_rdelivery_bytes: bad capacity %d or slot %d" % (self.cap, self.slot))
        self.buf = ctx.alloc(nbytes)
        self.desc = RDelivery()
        check(ctx.L.usn_rdelivery_bind(self.buf.ptr, nbytes, self.cap, self.slot, C.byref(self.desc)),
              "usn_rdelivery_bind")
        if poison is not None:
            check(ctx.L.usn_memset_d(ctx.h, self.buf.ptr, poison, nbytes, None), "usn_memset_d")
            ctx.sync()

    def info(self, stream=None, strict=True) -> DeliveryHdr:
        h = DeliveryHdr()
        rc = self.ctx.L.usn_deliver_round_info(self.ctx.h, C.byref(self.desc), stream, C.byref(h))
        if strict or rc != USN_ERANGE:
            check(rc, "usn_deliver_round_info")
        h.status = rc
        return h

    def seg_off(self) -> np.ndarray:
        """all USN_ROUND_MAX * (USN_MAX_ENDPOINTS + 1) + 1 segment offsets"""
        return self._get(self.desc.seg_off, np.uint32, USN_ROUND_MAX * (USN_MAX_ENDPOINTS + 1) + 1)

    def ring(self, e: int):
        """(src_idx, lens, bytes[k, slot], ring ids) of endpoint e's round ring;
        src_idx counts inside the slot's own ring"""
        so = self.seg_off()[USN_ROUND_MAX * e:USN_ROUND_MAX * (e + 1) + 1].astype(np.int64)
        k0, k1 = int(so[0]), int(so[-1])
        rings = np.repeat(np.arange(USN_ROUND_MAX, dtype=np.uint8), np.diff(so))
        return self.src(k0, k1), self.lens(k0, k1), self.slots(k0, k1), rings


class DeviceRingSet:
    """One usn_ringset: a circular ring of ring_slots[e] slots (0 or a power of
    two) of `slot` bytes per endpoint id e, with free-running head / tail
    counters.  `poison` fills the whole allocation before usn_ringset_init."""

    def __init__(self, ctx: Ctx, ring_slots, slot: int, poison: int | None = None):
        self.ctx = ctx
        sizes = np.ascontiguousarray(ring_slots, dtype=np.uint32)
        self.total = self.cap = max(int(sizes.astype(np.int64).sum()), 1)   # cap: DeviceDelivery's readers
        self.slot = int(slot)
        nbytes = ctx.L.usn_ringset_bytes(self.total, self.slot)
        if nbytes == 0:
            raise UsnError("usn_ringset_bytes: bad total %d or slot %d" % (self.total, self.slot))
        self.buf = ctx.alloc(nbytes)
        self.desc = RingSet()
        check(ctx.L.usn_ringset_bind(self.buf.ptr, nbytes, self.total, self.slot, C.byref(self.desc)),
              "usn_ringset_bind")
        if poison is not None:
            check(ctx.L.usn_memset_d(ctx.h, self.buf.ptr, poison, nbytes, None), "usn_memset_d")
            ctx.sync()
        check(ctx.L.usn_ringset_init(ctx.h, C.byref(self.desc), sizes.ctypes.data, sizes.size, None),
              "usn_ringset_init")
        self.off = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])   # ring e: [off[e], off[e + 1])

    def set_head(self, head, stream=None):
        """absolute head counters of ids 0 .. len(head) - 1 (usn_ringset_set_head)"""
        head = np.ascontiguousarray(head, dtype=np.uint32)
        check(self.ctx.L.usn_ringset_set_head(self.ctx.h, C.byref(self.desc), head.ctypes.data,
                                              head.size, stream), "usn_ringset_set_head")

    def set_counters(self, head, tail):
        """head and tail of ids 0 .. len - 1 by a plain device copy (tests and tools)"""
        for ptr, v in ((self.desc.head, head), (self.desc.tail, tail)):
            self.buf.upload(np.ascontiguousarray(v, dtype=np.uint32), offset=ptr - self.buf.ptr)

    def info(self, stream=None, strict=True) -> RingSetHdr:
        """The header after the call on `stream` finished.  strict: raise on
        USN_DV_DROPPED / USN_DV_LONG (USN_ERANGE); else return it with .status."""
        h = RingSetHdr()
        rc = self.ctx.L.usn_deliver_rings_info(self.ctx.h, C.byref(self.desc), stream, C.byref(h))
        if strict or rc != USN_ERANGE:
            check(rc, "usn_deliver_rings_info")
        h.status = rc
        return h

    _get = DeviceDelivery._get

    def _ids(self, ptr) -> np.ndarray:
        return self._get(ptr, np.uint32, USN_MAX_ENDPOINTS + 1)

    def head(self) -> np.ndarray:
        return self._ids(self.desc.head)

    def tail(self) -> np.ndarray:
        return self._ids(self.desc.tail)

    def first(self) -> np.ndarray:
        return self._ids(self.desc.first)

    def acc(self) -> np.ndarray:
        return self._ids(self.desc.acc)

    def drop(self) -> np.ndarray:
        return self._ids(self.desc.drop)

    def seg_acc(self) -> np.ndarray:
        """[id, ring]: accepted frames of segment (e, k) in the last call"""
        return self._get(self.desc.seg_acc, np.uint32,
                         USN_ROUND_MAX * (USN_MAX_ENDPOINTS + 1)).reshape(-1, USN_ROUND_MAX)

    lens, src, slots = DeviceDelivery.lens, DeviceDelivery.src, DeviceDelivery.slots   # of slots [k0, k1)

    def ring(self, e: int):
        """(lens, src_idx, bytes[k, slot]) of ring e from head to tail, in consumer order"""
        k0, k1 = int(self.off[e]), int(self.off[e + 1])
        h, t = int(self.head()[e]), int(self.tail()[e])
        pos = (h + np.arange(min((t - h) & 0xFFFFFFFF, k1 - k0), dtype=np.int64)) & (k1 - k0 - 1)
        return self.lens(k0, k1)[pos], self.src(k0, k1)[pos], self.slots(k0, k1)[pos]

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None


class DeviceBRingSet:
    """One usn_bringset: per endpoint id e a descriptor ring of ring_desc[e]
    entries and a byte ring of ring_units[e] 16-byte units (each 0 or a power of
    two, both or neither), free-running head / tail / btail.  `poison` fills
    the whole allocation before usn_bringset_init."""

    def __init__(self, ctx: Ctx, ring_desc, ring_units, poison: int | None = None):
        self.ctx = ctx
        D = np.ascontiguousarray(ring_desc, dtype=np.uint32)
        B = np.ascontiguousarray(ring_units, dtype=np.uint32)
        assert D.size == B.size
        self.total_desc = max(int(D.astype(np.int64).sum()), 1)
        self.total_units = max(int(B.astype(np.int64).sum()), 1)
        self.nbytes = ctx.L.usn_bringset_bytes(self.total_desc, self.total_units)
        if self.nbytes == 0:
            raise UsnError("usn_bringset_bytes: bad totals %d, %d" % (self.total_desc, self.total_units))
        self.buf = ctx.alloc(self.nbytes)
        self.desc = BRingSet()
        check(ctx.L.usn_bringset_bind(self.buf.ptr, self.nbytes, self.total_desc, self.total_units,
                                      C.byref(self.desc)), "usn_bringset_bind")
        if poison is not None:
            check(ctx.L.usn_memset_d(ctx.h, self.buf.ptr, poison, self.nbytes, None), "usn_memset_d")
            ctx.sync()
        check(ctx.L.usn_bringset_init(ctx.h, C.byref(self.desc), D.ctypes.data, B.ctypes.data, D.size, None),
              "usn_bringset_init")
        self.doff = np.concatenate([[0], np.cumsum(D.astype(np.int64))])   # descriptors of e: [doff[e], doff[e + 1])
        self.uoff = np.concatenate([[0], np.cumsum(B.astype(np.int64))])   # units of e: [uoff[e], uoff[e + 1])

    def set_head(self, head, stream=None):
        """absolute head counters of ids 0 .. len(head) - 1 (usn_bringset_set_head)"""
        head = np.ascontiguousarray(head, dtype=np.uint32)
        check(self.ctx.L.usn_bringset_set_head(self.ctx.h, C.byref(self.desc), head.ctypes.data,
                                               head.size, stream), "usn_bringset_set_head")

    def set_counters(self, head, tail, btail):
        """head, tail and btail of ids 0 .. len - 1 by a plain device copy (tests and tools)"""
        for ptr, v in ((self.desc.head, head), (self.desc.tail, tail), (self.desc.btail, btail)):
            self.buf.upload(np.ascontiguousarray(v, dtype=np.uint32), offset=ptr - self.buf.ptr)

    def info(self, stream=None, strict=True) -> BRingSetHdr:
        """The header after the call on `stream` finished.  strict: raise on
        USN_DV_DROPPED (USN_ERANGE); else return it with .status."""
        h = BRingSetHdr()
        rc = self.ctx.L.usn_deliver_brings_info(self.ctx.h, C.byref(self.desc), stream, C.byref(h))
        if strict or rc != USN_ERANGE:
            check(rc, "usn_deliver_brings_info")
        h.status = rc
        return h

    _get = DeviceDelivery._get

    def _ids(self, ptr) -> np.ndarray:
        return self._get(ptr, np.uint32, USN_MAX_ENDPOINTS + 1)

    def head(self) -> np.ndarray:
        return self._ids(self.desc.head)

    def tail(self) -> np.ndarray:
        return self._ids(self.desc.tail)

    def btail(self) -> np.ndarray:
        return self._ids(self.desc.btail)

    def first(self) -> np.ndarray:
        return self._ids(self.desc.first)

    def bfirst(self) -> np.ndarray:
        return self._ids(self.desc.bfirst)

    def acc(self) -> np.ndarray:
        return self._ids(self.desc.acc)

    def drop(self) -> np.ndarray:
        return self._ids(self.desc.drop)

    def acc_units(self) -> np.ndarray:
        return self._ids(self.desc.acc_units)

    def seg_acc(self) -> np.ndarray:
        """[id, ring]: accepted frames of segment (e, k) in the last call"""
        return self._get(self.desc.seg_acc, np.uint32,
                         USN_ROUND_MAX * (USN_MAX_ENDPOINTS + 1)).reshape(-1, USN_ROUND_MAX)

    def desc_off(self) -> np.ndarray:
        return self._get(self.desc.desc_off, np.uint32, USN_MAX_ENDPOINTS + 2)

    def unit_off(self) -> np.ndarray:
        return self._get(self.desc.unit_off, np.uint32, USN_MAX_ENDPOINTS + 2)

    def lens(self) -> np.ndarray:
        return self._get(self.desc.lens, np.uint16, self.total_desc)

    def src(self) -> np.ndarray:
        return self._get(self.desc.src, np.uint32, self.total_desc)

    def pos16(self) -> np.ndarray:
        return self._get(self.desc.pos16, np.uint32, self.total_desc)

    def units(self) -> np.ndarray:
        """all of frames, as [total_units, 16]"""
        return self._get(self.desc.frames, np.uint8, self.total_units * 16).reshape(-1, 16)

    def ring(self, e: int):
        """(lens, src_idx, [bytes of ceil16(len) per frame]) of ring e from head to
        tail, in consumer order, both rings unwrapped"""
        d0, D = int(self.doff[e]), int(self.doff[e + 1] - self.doff[e])
        u0, B = int(self.uoff[e]), int(self.uoff[e + 1] - self.uoff[e])
        h, t = int(self.head()[e]), int(self.tail()[e])
        q = d0 + ((h + np.arange(min((t - h) & 0xFFFFFFFF, D), dtype=np.int64)) & (D - 1))
        lens, src, pos, units = self.lens()[q], self.src()[q], self.pos16()[q], self.units()
        body = [units[u0 + ((int(p) + np.arange(max(1, (int(ln) + 15) // 16))) & (B - 1))].reshape(-1)
                for p, ln in zip(pos, lens)]
        return lens, src, body

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None


class DevicePackedDelivery:
    """One usn_pdelivery: cap_bytes of frames lying back to back (each padded to
    16 bytes), off16[] / lens[] / src[] per slot, the per-endpoint slot and byte
    offsets and the header.  `poison` as for DeviceDelivery."""

    def __init__(self, ctx: Ctx, cap_slots: int, cap_bytes: int, poison: int | None = None):
        self.ctx = ctx
        self.cap = int(cap_slots)
        self.cap_bytes = int(cap_bytes)
        nbytes = ctx.L.usn_pdelivery_bytes(self.cap, self.cap_bytes)
        if nbytes == 0:
            raise UsnError("usn_pdelivery_bytes: bad capacity %d slots / %d bytes" % (self.cap, self.cap_bytes))
        self.buf = ctx.alloc(nbytes)
        self.desc = PDelivery()
        check(ctx.L.usn_pdelivery_bind(self.buf.ptr, nbytes, self.cap, self.cap_bytes,
                                       C.byref(self.desc)), "usn_pdelivery_bind")
        if poison is not None:
            check(ctx.L.usn_memset_d(ctx.h, self.buf.ptr, poison, nbytes, None), "usn_memset_d")
            ctx.sync()

    def info(self, stream=None, strict=True) -> PDeliveryHdr:
        """The header after the delivery on `stream` finished.  strict: raise on
        either overflow flag (USN_ERANGE); else return it with .status."""
        h = PDeliveryHdr()
        rc = self.ctx.L.usn_deliver_packed_info(self.ctx.h, C.byref(self.desc), stream, C.byref(h))
        if strict or rc != USN_ERANGE:
            check(rc, "usn_deliver_packed_info")
        h.status = rc
        return h

    _get = DeviceDelivery._get

    def ep_off(self) -> np.ndarray:
        """slots of endpoint e = [ep_off[e], ep_off[e + 1])"""
        return self._get(self.desc.ep_off, np.uint32, USN_MAX_ENDPOINTS + 1)

    def ep_boff(self) -> np.ndarray:
        """bytes of endpoint e = [ep_boff[e], ep_boff[e + 1])"""
        return self._get(self.desc.ep_boff, np.uint64, USN_MAX_ENDPOINTS + 1)

    def src(self, k0=0, k1=None) -> np.ndarray:
        k1 = self.cap if k1 is None else k1
        return self._get(self.desc.src + 4 * k0, np.uint32, k1 - k0)

    def lens(self, k0=0, k1=None) -> np.ndarray:
        k1 = self.cap if k1 is None else k1
        return self._get(self.desc.lens + 2 * k0, np.uint16, k1 - k0)

    def off16(self, k0=0, k1=None) -> np.ndarray:
        """start of slot k's frame in 16-byte units"""
        k1 = self.cap if k1 is None else k1
        return self._get(self.desc.off16 + 4 * k0, np.uint32, k1 - k0)

    def bytes(self, b0=0, b1=None) -> np.ndarray:
        """frames[b0, b1) (default: the whole region of cap_bytes)"""
        b1 = self.cap_bytes if b1 is None else b1
        return self._get(self.desc.frames + b0, np.uint8, b1 - b0)

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None


class DeviceDrain:
    """One usn_drain: what a usn_rings_drain call takes out of a ring set (or a
    usn_brings_drain call out of a byte ring set) --
    cap_bytes of frames lying back to back (each padded to 16 bytes), off16[] /
    lens[] / src[] per output slot, the per-id slot and byte offsets, the
    budgets (input), from / take / left per id and the header.  `poison` as for
    DeviceDelivery; the budgets start at 0 either way."""

    def __init__(self, ctx: Ctx, cap_slots: int, cap_bytes: int, poison: int | None = None):
        self.ctx = ctx
        self.cap = int(cap_slots)
        self.cap_bytes = int(cap_bytes)
        nbytes = ctx.L.usn_drain_bytes(self.cap, self.cap_bytes)
        if nbytes == 0:
            raise UsnError("usn_drain_bytes: bad capacity %d slots / %d bytes" % (self.cap, self.cap_bytes))
        self.buf = ctx.alloc(nbytes)
        self.desc = Drain()
        check(ctx.L.usn_drain_bind(self.buf.ptr, nbytes, self.cap, self.cap_bytes, C.byref(self.desc)),
              "usn_drain_bind")
        if poison is not None:
            check(ctx.L.usn_memset_d(ctx.h, self.buf.ptr, poison, nbytes, None), "usn_memset_d")
            ctx.sync()
        self.set_budget([])

    def set_budget(self, budget, stream=None):
        """the most frames to take from ring 0 .. len(budget) - 1 per call; the other ids get 0"""
        budget = np.ascontiguousarray(budget, dtype=np.uint32)
        check(self.ctx.L.usn_drain_set_budget(self.ctx.h, C.byref(self.desc), budget.ctypes.data,
                                              budget.size, stream), "usn_drain_set_budget")

    def info(self, stream=None, strict=True, brings=False) -> DrainHdr:
        """The header after the drain on `stream` finished.  strict: raise on
        USN_DV_OVERFLOW_BYTES / USN_DR_BADCOUNT (USN_ERANGE); else return it with .status.
        brings: the call was usn_brings_drain (USN_DR_BADDESC is USN_ERANGE too)."""
        h = DrainHdr()
        name = "usn_brings_drain_info" if brings else "usn_rings_drain_info"
        rc = getattr(self.ctx.L, name)(self.ctx.h, C.byref(self.desc), stream, C.byref(h))
        if strict or rc != USN_ERANGE:
            check(rc, name)
        h.status = rc
        return h

    _get = DeviceDelivery._get

    def ep_off(self) -> np.ndarray:
        """slots of id e = [ep_off[e], ep_off[e + 1]), e <= USN_MAX_ENDPOINTS"""
        return self._get(self.desc.ep_off, np.uint32, USN_MAX_ENDPOINTS + 2)

    def ep_boff(self) -> np.ndarray:
        """bytes of id e = [ep_boff[e], ep_boff[e + 1])"""
        return self._get(self.desc.ep_boff, np.uint64, USN_MAX_ENDPOINTS + 2)

    def _ids(self, ptr) -> np.ndarray:
        return self._get(ptr, np.uint32, USN_MAX_ENDPOINTS + 1)

    def from_(self) -> np.ndarray:
        return self._ids(self.desc.from_)

    def take(self) -> np.ndarray:
        return self._ids(self.desc.take)

    def left(self) -> np.ndarray:
        return self._ids(self.desc.left)

    # the output arrays are usn_pdelivery's
    src, lens, off16 = DevicePackedDelivery.src, DevicePackedDelivery.lens, DevicePackedDelivery.off16
    bytes, free = DevicePackedDelivery.bytes, DevicePackedDelivery.free
