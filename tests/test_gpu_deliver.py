"""usn_deliver: every receiver's output ring, packed on the device, against a
numpy restatement of the rule (usn_classify.h "delivery") applied to the
decisions the same result holds.  ep_off, src[], lens[] and the slot bytes
[0, ceil16(len)) are bit-exact; what lies past them keeps the test's poison.

Endpoints: NIC 0, host ring 1, pipes 2-4 (for_nic 0).  UDP to port 1000 + e is
ruled to endpoint e (EP bins), ARP / EAPOL flood, other UDP drops, and a frame
a pipe sends to a MAC outside the bridge goes to its NIC.  A real NIC never
owns a rule, so its ring merges two lists (NIC + FLOOD); the `nic_is_pipe`
case re-registers id 0 as a pipe that owns a rule, which makes ring 0 the
three-way merge own + NIC + FLOOD.
"""
import numpy as np
import pytest

from usnetd_amd import lib

pytestmark = pytest.mark.gpu
P = lib.USN_DELIVER_TILE
POISON = 0xEE
EP, ARP, EAPOL, DROP, NIC = 0, 16, 17, 18, 19   # frame kinds; EP + e: ruled to endpoint e


def expected(dec, regs, src, nic):
    """per registered receiver: the frame indices it gets, ascending"""
    cls, ep = (dec >> 16) & 0xF, dec & 0xFFFF
    return {e: np.flatnonzero(((cls == lib.CLS_EP) & (ep == e)) | ((cls == lib.CLS_NIC) & (e == nic)) |
                              ((cls == lib.CLS_FLOOD) & (e != src))) for e in regs}


def build(kinds, lens, starts, src, poison_to=0):
    """the frames' bytes (flat, padded) for these kinds, lengths and starts;
    poison_to: bytes [len, poison_to) of every input slot are 0xA5"""
    rng = np.random.default_rng(len(kinds))
    F = rng.integers(0, 256, int(starts[-1]) + 2048, dtype=np.uint8)
    for i, (k, ln, s) in enumerate(zip(kinds, lens, starts)):
        s = int(s)
        dmac = bytes([2, 0x99, 0, 0, 0, 1]) if k == NIC else bytes([2, 0, 0, 0, 0, k if k < 16 else 3])
        h = dmac + bytes([2, 0, 0, 0, 0, src])
        if k in (ARP, EAPOL):
            h += b"\x08\x06" if k == ARP else b"\x88\x8e"
        else:
            port = 1000 + k if k < 16 else 9
            h += (b"\x08\x00" + bytes([0x45, 0, 0, 46, 0, i & 255, 0x40, 0, 64, 17, 0, 0, 10, 0, 1, 1,
                                       10, 0, 0, 2, 0x10, i % 50, port >> 8, port & 255, 0, 26, 0, 0]))
        F[s:s + len(h)] = np.frombuffer(h, np.uint8)
        F[s + int(ln):s + poison_to] = 0xA5
    return F


def setup(kinds, src=0, stride=64, lens=None, offsets=False, nic_is_pipe=False, poison_in=False):
    n = len(kinds)
    kinds = np.asarray(kinds)
    if lens is None:
        lens = np.where(kinds == ARP, 42, np.where(kinds == EAPOL, 22, 60))
    lens = np.asarray(lens, np.uint16)
    kinds = np.where((lens < 60) & (kinds != EAPOL), ARP, kinds)   # a short frame parses only as ARP / EAPOL
    sizes = (lens.astype(np.int64) + 15) // 16 * 16 + 16   # offsets[]: 16-byte aligned, a gap between frames
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if offsets else np.arange(n, dtype=np.int64) * stride
    F = build(kinds, lens, starts, src, poison_to=stride if poison_in else 0)
    ctx = lib.Ctx(0)
    ctx.endpoint_add(0, lib.EP_NIC)
    ctx.endpoint_add(1, lib.EP_HOST, 0)
    for e in (2, 3, 4):
        ctx.endpoint_add(e, lib.EP_PIPE, 0)
        ctx.bridge_add(bytes([2, 0, 0, 0, 0, e]))
    owners = [1, 2, 3, 4]
    if nic_is_pipe:   # id 0 again, as a pipe of another NIC: the senders' for_nic still names it
        ctx.endpoint_add(6, lib.EP_NIC)
        ctx.endpoint_remove(0)
        ctx.endpoint_add(0, lib.EP_PIPE, 6)
        ctx.bridge_add(bytes([2, 0, 0, 0, 0, 0]))
        owners = [0] + owners
    for e in owners:
        ctx.add_match(lib.make_want("10.0.0.2", 17, 1000 + e), e)
    s = ctx.stream()
    b = lib.DeviceBatch(ctx, F, lens, src, stride=0 if offsets else stride,
                        offsets=starts.astype(np.uint64) if offsets else None)
    r = lib.DeviceResult(ctx, n)
    ctx.classify(b, r, s)
    ctx.finalize(b, r, s)
    return ctx, s, b, r, r.decisions(), F, lens, starts


def deliver_and_check(ctx, s, b, r, dec, F, lens, starts, slot, regs, src, nic=0, cap_extra=3):
    want = expected(dec, regs, src, nic)
    counts = np.zeros(lib.USN_MAX_ENDPOINTS, np.int64)
    for e, w in want.items():
        counts[e] = w.size
    need = int(counts.sum())
    dv = lib.DeviceDelivery(ctx, need + cap_extra, slot, poison=POISON)
    ctx.deliver(b, r, dv, s)
    hdr = dv.info(s, strict=False)
    long_ = bool((lens[np.concatenate([want[e] for e in sorted(want)])] > slot).any()) if need else False
    assert (hdr.need, hdr.n_recv, hdr.cap) == (need, int((counts > 0).sum()), need + cap_extra)
    assert hdr.flags == (lib.DV_LONG if long_ else 0) and hdr.status == (lib.USN_ERANGE if long_ else 0)
    np.testing.assert_array_equal(dv.ep_off(), np.concatenate([[0], np.cumsum(counts)]))
    idx = np.concatenate([want[e] for e in sorted(want)] + [np.zeros(0, np.int64)])
    np.testing.assert_array_equal(dv.src()[:need], idx)
    np.testing.assert_array_equal(dv.lens()[:need], lens[idx])
    assert (dv.src()[need:] == POISON * 0x01010101).all() and (dv.lens()[need:] == POISON * 0x0101).all()
    col = np.arange(slot)
    L = lens[idx].astype(np.int64)[:, None]
    body = F[starts[idx][:, None] + col]
    exp = np.where(col < L, body, np.where(col < (L + 15) // 16 * 16, 0, POISON)).astype(np.uint8)
    got = dv.slots()
    np.testing.assert_array_equal(got[:need], exp)
    assert (got[need:] == POISON).all()
    dv.free()
    return want


def rx_kinds(n):
    """mostly endpoint 1 (the largest ring), the others and drops sprinkled in;
    FLOOD at frames 0 and n - 1 and on both sides of every tile cut of ring 1"""
    k = np.full(n, EP + 1)
    k[3::7], k[4::11], k[5::13], k[6::17] = EP + 2, EP + 3, EP + 4, DROP
    k[0], k[n - 1] = ARP, EAPOL
    ring1 = np.flatnonzero((k == EP + 1) | (k >= ARP) & (k <= EAPOL))
    for j in range(P, ring1.size, P):
        k[ring1[j - 1:j + 1]] = ARP
    return k


@pytest.mark.parametrize("n", [1, 1023, 1025, 3 * P + 1])
def test_rx_merge_and_tile_cuts(n):
    st = setup(rx_kinds(n))
    want = deliver_and_check(*st, slot=64, regs=range(5), src=0)
    assert want[0].size == 0 and all(want[e].size for e in range(1, 5))
    st[0].close()


@pytest.mark.parametrize("nic_is_pipe", [False, True])
def test_tx_merge(nic_is_pipe):
    """pipe 2 sends 2P + 3 frames; ring 0 alternates among NIC, FLOOD (and, with
    id 0 a rule-owning pipe, its own bin) across a tile cut"""
    n = 2 * P + 3
    cyc = [EP + 3, NIC, ARP, EP + 0 if nic_is_pipe else EP + 4, NIC, EAPOL, DROP]
    st = setup([cyc[i % 7] for i in range(n)], src=2, nic_is_pipe=nic_is_pipe)
    dec = st[4]
    regs = [0, 1, 2, 3, 4] + ([6] if nic_is_pipe else [])
    want = deliver_and_check(*st, slot=64, regs=regs, src=2)
    cls0 = set(((dec[want[0]] >> 16) & 0xF).tolist())
    assert cls0 == ({lib.CLS_EP, lib.CLS_NIC, lib.CLS_FLOOD} if nic_is_pipe else {lib.CLS_NIC, lib.CLS_FLOOD})
    assert want[0].size > P and want[2].size == 0
    st[0].close()


def test_lengths_and_tail_masking():
    """slot 128: every length around the 16-byte pieces; the input slot past len is 0xA5"""
    pool = np.array([14, 15, 16, 17, 31, 32, 33, 60, 64, 65, 127, 128])
    n = 600
    lens = pool[np.random.default_rng(3).integers(0, pool.size, n)]
    st = setup([EP + 1 + i % 4 if i % 3 else ARP for i in range(n)], stride=128, lens=lens, poison_in=True)
    deliver_and_check(*st, slot=128, regs=range(5), src=0)
    st[0].close()


def test_multi_pass_copy_offsets_layout():
    """slot 1536 (64 lanes per frame, two passes), frames at 16-byte aligned offsets[]"""
    n = 300
    lens = np.array([60, 1024, 1025, 1514])[np.random.default_rng(4).integers(0, 4, n)]
    st = setup([EP + 1 + i % 4 if i % 5 else EAPOL for i in range(n)], lens=lens, offsets=True)
    deliver_and_check(*st, slot=1536, regs=range(5), src=0)
    deliver_and_check(*st, slot=1024, regs=range(5), src=0)   # truncated: USN_DV_LONG
    st[0].close()


def test_receiver_set_follows_the_context():
    st = setup(rx_kinds(1025))
    ctx = st[0]
    deliver_and_check(*st, slot=64, regs=range(5), src=0)
    ctx.endpoint_remove(3)
    ctx.endpoint_add(5, lib.EP_PIPE, 0)
    want = deliver_and_check(*st, slot=64, regs=[0, 1, 2, 4, 5], src=0)
    dec = st[4]
    assert ((dec & 0xFFFF) == 3).any()   # endpoint 3's bin is not empty; its ring is
    np.testing.assert_array_equal(want[5], np.flatnonzero((dec >> 16) & 0xF == lib.CLS_FLOOD))
    ctx.close()


def test_capacity_overflow_writes_nothing():
    ctx, s, b, r, dec, F, lens, starts = st = setup(rx_kinds(1025))
    want = expected(dec, range(5), 0, 0)
    need = sum(w.size for w in want.values())
    dv = lib.DeviceDelivery(ctx, need - 1, 64, poison=POISON)
    ctx.deliver(b, r, dv, s)
    hdr = dv.info(s, strict=False)
    assert hdr.status == lib.USN_ERANGE and hdr.need == need and hdr.flags == lib.DV_OVERFLOW
    np.testing.assert_array_equal(dv.ep_off()[:6], np.cumsum([0] + [want[e].size for e in range(5)]))
    assert (dv.slots() == POISON).all() and (dv.lens() == POISON * 0x0101).all()
    assert (dv.src() == POISON * 0x01010101).all()
    deliver_and_check(*st, slot=64, regs=range(5), src=0, cap_extra=0)
    ctx.close()
