"""usn_deliver_round: one ring per endpoint for a whole poll round, against the
numpy restatement of the receiver rule that test_gpu_deliver.py uses, applied
to each ring's own decisions and concatenated per receiver in ring order.
seg_off, ep_off, src[], lens[] and the slot bytes [0, ceil16(len)) are
bit-exact; what lies past those bytes, and past need, keeps the poison.

Endpoints as in test_gpu_deliver.py: NIC 0, host 1, pipes 2-4; `pipe0` makes
id 0 a rule-owning pipe of NIC 6 (its nic_is_pipe).  A ring is (kinds, src,
layout options); all rings of a case live in one context.
"""
import numpy as np
import pytest

from usnetd_amd import lib
import test_gpu_deliver as base
from test_gpu_deliver import ARP, DROP, EAPOL, EP, NIC, P, POISON

pytestmark = pytest.mark.gpu
RM = lib.USN_ROUND_MAX
IDS = lib.USN_MAX_ENDPOINTS + 1
TX_CYCLE = [EP + 3, NIC, ARP, EP + 0, NIC, EAPOL, DROP]   # test_tx_merge's, nic_is_pipe


def make_ctx(pipe0=False):
    ctx = lib.Ctx(0)
    ctx.endpoint_add(0, lib.EP_NIC)
    ctx.endpoint_add(1, lib.EP_HOST, 0)
    for e in (2, 3, 4):
        ctx.endpoint_add(e, lib.EP_PIPE, 0)
    if pipe0:
        ctx.endpoint_add(6, lib.EP_NIC)
        ctx.endpoint_remove(0)
        ctx.endpoint_add(0, lib.EP_PIPE, 6)
    for e in ([0] if pipe0 else []) + [1, 2, 3, 4]:
        if e != 1:
            ctx.bridge_add(bytes([2, 0, 0, 0, 0, e]))
        ctx.add_match(lib.make_want("10.0.0.2", 17, 1000 + e), e)
    return ctx, ctx.stream(), ([0, 1, 2, 3, 4, 6] if pipe0 else [0, 1, 2, 3, 4])


def add_ring(ctx, s, kinds, src=0, stride=64, lens=None, offsets=False, poison_in=False, finalize=True):
    """base.setup's batch, classified in this context: (b, r, F, lens, starts, src)"""
    kinds = np.asarray(kinds)
    if lens is None:
        lens = np.where(kinds == ARP, 42, np.where(kinds == EAPOL, 22, 60))
    lens = np.asarray(lens, np.uint16)
    kinds = np.where((lens < 60) & (kinds != EAPOL), ARP, kinds)
    sizes = (lens.astype(np.int64) + 15) // 16 * 16 + 16
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if offsets else np.arange(kinds.size, dtype=np.int64) * stride
    F = base.build(kinds, lens, starts, src, poison_to=stride if poison_in else 0)
    b = lib.DeviceBatch(ctx, F, lens, src, stride=0 if offsets else stride,
                        offsets=starts.astype(np.uint64) if offsets else None)
    r = lib.DeviceResult(ctx, kinds.size)
    ctx.classify(b, r, s)
    if finalize:
        ctx.finalize(b, r, s)
    return b, r, F, lens, starts, src


def reference(rings, regs, pipe0):
    """want[k][e]: ring k's frames for receiver e; seg[e, k] their count"""
    want = [base.expected(r.decisions(), regs, src, (6 if src == 0 else 0) if pipe0 else 0)
            for _, r, _, _, _, src in rings]
    seg = np.zeros((IDS, RM), np.int64)
    for k, w in enumerate(want):
        for e, idx in w.items():
            seg[e, k] = idx.size
    return want, seg


def deliver_and_check(ctx, s, rings, regs, slot, pipe0=False, cap_delta=3):
    want, seg = reference(rings, regs, pipe0)
    seg_off = np.concatenate([[0], np.cumsum(seg.reshape(-1))])
    need, cap = int(seg_off[-1]), int(seg_off[-1]) + cap_delta
    dv = lib.DeviceRoundDelivery(ctx, cap, slot, poison=POISON)
    ctx.deliver_round([g[0] for g in rings], [g[1] for g in rings], dv, s)
    hdr = dv.info(s, strict=False)
    order = [(e, k) for e in sorted(regs) for k in range(len(rings))]
    src = np.concatenate([want[k][e] for e, k in order] + [np.zeros(0, np.int64)])
    lens = np.concatenate([rings[k][3][want[k][e]] for e, k in order] + [np.zeros(0, np.uint16)])
    long_ = bool((lens > slot).any())
    print("need %d, segments of receiver 0: %s, of receiver 1: %s, flags %d" % (hdr.need, seg[0], seg[1], hdr.flags))
    assert (hdr.need, hdr.n_recv, hdr.cap) == (need, int((seg.sum(1) > 0).sum()), cap)
    np.testing.assert_array_equal(dv.seg_off(), seg_off)
    np.testing.assert_array_equal(dv.ep_off(), seg_off[::RM][:IDS])
    if need > cap:   # nothing but the plan's arrays is written
        assert hdr.flags == lib.DV_OVERFLOW and hdr.status == lib.USN_ERANGE
        need = 0
    else:
        assert hdr.flags == (lib.DV_LONG if long_ else 0) and hdr.status == (lib.USN_ERANGE if long_ else 0)
    np.testing.assert_array_equal(dv.src()[:need], src[:need])
    np.testing.assert_array_equal(dv.lens()[:need], lens[:need])
    assert (dv.src()[need:] == POISON * 0x01010101).all() and (dv.lens()[need:] == POISON * 0x0101).all()
    col = np.arange(slot)
    body = [rings[k][2][rings[k][4][want[k][e]][:, None] + col] for e, k in order if want[k][e].size]
    L = lens[:need].astype(np.int64)[:, None]
    exp = np.where(col < L, np.concatenate(body + [np.zeros((0, slot), np.uint8)])[:need],
                   np.where(col < (L + 15) // 16 * 16, 0, POISON)).astype(np.uint8)
    got = dv.slots()
    np.testing.assert_array_equal(got[:need], exp)
    assert (got[need:] == POISON).all()
    if need:
        rid = np.concatenate([np.full(want[k][1].size, k) for k in range(len(rings))])
        np.testing.assert_array_equal(dv.ring(1)[3], rid)
    dv.free()
    return want, seg


def test_one_ring_equals_usn_deliver():
    ctx, s, regs = make_ctx()
    ring = add_ring(ctx, s, base.rx_kinds(1025))
    _, seg = deliver_and_check(ctx, s, [ring], regs, 64)
    cap = int(seg.sum()) + 3
    dv, rv = lib.DeviceDelivery(ctx, cap, 64, poison=POISON), lib.DeviceRoundDelivery(ctx, cap, 64, poison=POISON)
    ctx.deliver(ring[0], ring[1], dv, s)
    ctx.deliver_round([ring[0]], [ring[1]], rv, s)
    assert bytes(dv.info(s)) == bytes(rv.info(s))
    for f in ("ep_off", "src", "lens", "slots"):
        np.testing.assert_array_equal(getattr(dv, f)(), getattr(rv, f)())
    so = rv.seg_off()[:-1].reshape(IDS, RM)
    assert (so[:, 1:] == so[:, 1:2]).all()
    ctx.close()


def test_tile_across_segment_ends():
    ctx, s, regs = make_ctx()
    rings = [add_ring(ctx, s, base.rx_kinds(1023)),
             add_ring(ctx, s, [ARP, EP + 1, EAPOL, NIC, EP + 3, ARP, DROP], src=2),
             add_ring(ctx, s, base.rx_kinds(2 * P + 5))]
    _, seg = deliver_and_check(ctx, s, rings, regs, 64)
    a, b = seg[1, 0], seg[1, 0] + seg[1, 1]
    assert P < a and seg[1, 1] > 0 and b < 2 * P and b % P != 0   # tile 1: the end of 0, all of 1, the start of 2
    assert seg[1].sum() > 2 * P                                    # ... and ring 2 is cut again, off the tile grid
    ctx.close()


@pytest.mark.parametrize("side_src", [0, 3])
def test_three_list_cut_at_an_unaligned_position(side_src):
    """receiver 0's middle segment merges own + NIC + FLOOD over more than a tile.  A sender gets
    nothing from its own ring: sent by id 0 the outer rings leave that segment on a tile start;
    sent by pipe 3 they come first in ring 0 and the three lists are entered, and cut, off the grid"""
    ctx, s, regs = make_ctx(pipe0=True)
    side = [[EP + 0, EP + 1, ARP, EP + 0, EP + 3][i % 5] for i in range(300)]
    rings = [add_ring(ctx, s, side, src=side_src),
             add_ring(ctx, s, [TX_CYCLE[i % 7] for i in range(2 * P + 3)], src=2),
             add_ring(ctx, s, side, src=side_src)]
    want, seg = deliver_and_check(ctx, s, rings, regs, 64, pipe0=True)
    cls = set(((rings[1][1].decisions()[want[1][0]] >> 16) & 0xF).tolist())
    assert cls == {lib.CLS_EP, lib.CLS_NIC, lib.CLS_FLOOD} and seg[0, 1] > P
    assert (seg[0, 0] == seg[0, 2] == 0) if side_src == 0 else (0 < seg[0, 0] < P and seg[0, 2] > 0)
    ctx.close()


def test_eight_short_rings():
    ctx, s, regs = make_ctx()
    kinds = [[EP + 1], [ARP, EP + 3], [EP + 2, EP + 2, DROP], [NIC], [ARP], [EP + 1, EAPOL, NIC], [DROP],
             [EP + 4, ARP]]
    rings = [add_ring(ctx, s, k, src=2 * (i % 2)) for i, k in enumerate(kinds)]
    want, seg = deliver_and_check(ctx, s, rings, regs, 64)
    assert (seg[:5].sum(1) < P).all() and ((seg[1:5] == 0).sum(1) >= 2).all()   # one tile each, with empty segments
    assert want[1][2].tolist() == [] and want[1][1].tolist() == [0] and want[4][0].tolist() == []   # no FLOOD to its sender
    ctx.close()


@pytest.mark.parametrize("slot", [1536, 128])
def test_mixed_layouts(slot):
    """stride 64, stride 128 poisoned past len, offsets[]; slot 1536: multi-pass copy, 128: USN_DV_LONG"""
    ctx, s, regs = make_ctx()
    rng = np.random.default_rng(7)
    pool = np.array([14, 15, 16, 17, 31, 32, 33, 60, 64, 65, 127, 128])
    rings = [add_ring(ctx, s, base.rx_kinds(200)),
             add_ring(ctx, s, [EP + 1 + i % 4 if i % 3 else ARP for i in range(300)], stride=128,
                      lens=pool[rng.integers(0, pool.size, 300)], poison_in=True),
             add_ring(ctx, s, [EP + 1 + i % 4 if i % 5 else EAPOL for i in range(100)], offsets=True,
                      lens=np.array([60, 1024, 1025, 1514])[rng.integers(0, 4, 100)])]
    deliver_and_check(ctx, s, rings, regs, slot)
    ctx.close()


def test_capacity_overflow_writes_nothing():
    ctx, s, regs = make_ctx()
    rings = [add_ring(ctx, s, base.rx_kinds(1025)), add_ring(ctx, s, base.rx_kinds(600))]
    deliver_and_check(ctx, s, rings, regs, 64, cap_delta=-1)
    deliver_and_check(ctx, s, rings, regs, 64, cap_delta=0)
    ctx.close()


def test_unfinalized_tx_ring_is_busy():
    ctx, s, regs = make_ctx()
    rings = [add_ring(ctx, s, base.rx_kinds(100)),
             add_ring(ctx, s, [TX_CYCLE[i % 7] for i in range(50)], src=2, finalize=False)]
    dv = lib.DeviceRoundDelivery(ctx, 1000, 64)
    with pytest.raises(lib.UsnError, match="EBUSY"):
        ctx.deliver_round([g[0] for g in rings], [g[1] for g in rings], dv, s)
    ctx.finalize(rings[1][0], rings[1][1], s)
    deliver_and_check(ctx, s, rings, regs, 64)
    ctx.close()
