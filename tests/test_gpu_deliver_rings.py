"""usn_deliver_rings: a poll round appended to persistent endpoint rings, bit-exact
against a plain model: per registered receiver test_gpu_deliver.expected(...) over
the rings in order, the frames written one by one into a numpy ring with head /
tail, a frame dropped when its ring is full.  After every call first, acc, drop,
seg_acc, tail and the header are compared, and lens / src / frames as WHOLE
arrays: the appended slots' bytes [0, ceil16(len)), and that everything else
keeps the poison or what an earlier call left there.
"""
import numpy as np
import pytest

from usnetd_amd import lib
import test_gpu_deliver as base
from test_gpu_deliver import ARP, DROP, EAPOL, EP, NIC, P, POISON
from test_gpu_deliver_round import TX_CYCLE, add_ring, make_ctx, reference

pytestmark = pytest.mark.gpu
RM, IDS, M32 = lib.USN_ROUND_MAX, lib.USN_MAX_ENDPOINTS + 1, 0xFFFFFFFF


class Model:
    def __init__(self, sizes, slot):
        self.size = np.zeros(IDS, np.int64)
        self.size[:len(sizes)] = sizes
        self.off = np.concatenate([[0], np.cumsum(self.size)])
        total = max(int(self.off[-1]), 1)
        self.slot, self.head, self.tail = slot, [0] * IDS, [0] * IDS
        self.lens = np.full(total, POISON * 0x0101, np.uint16)
        self.src = np.full(total, POISON * 0x01010101, np.uint32)
        self.frames = np.full((total, slot), POISON, np.uint8)

    def append(self, rings, regs, pipe0):
        want, _ = reference(rings, regs, pipe0)
        first, seg_acc, offered = np.array(self.tail), np.zeros((IDS, RM), np.int64), np.zeros(IDS, np.int64)
        long_ = False
        for e in regs:
            S = int(self.size[e])
            for k, (_, _, F, lens, starts, _) in enumerate(rings):
                for i in want[k][e]:
                    offered[e] += 1
                    if ((self.tail[e] - self.head[e]) & M32) >= S:
                        continue   # full (or a head ahead of the tail): this frame is lost
                    o, ln = int(self.off[e]) + (self.tail[e] & (S - 1)), int(lens[i])
                    w = min((ln + 15) // 16 * 16, self.slot)
                    self.frames[o, :w] = 0
                    self.frames[o, :min(ln, w)] = F[int(starts[i]):int(starts[i]) + min(ln, w)]
                    self.lens[o], self.src[o] = ln, i
                    self.tail[e] = (self.tail[e] + 1) & M32
                    seg_acc[e, k] += 1
                    long_ |= ln > self.slot
        acc = seg_acc.sum(1)
        return dict(first=first, seg_acc=seg_acc, acc=acc, drop=offered - acc, offered=int(offered.sum()),
                    flags=(lib.DV_LONG if long_ else 0) | (lib.DV_DROPPED if (offered > acc).any() else 0))


def new_set(ctx, sizes, slot=64):
    return lib.DeviceRingSet(ctx, sizes, slot, poison=POISON), Model(sizes, slot)


def set_counters(rs, mo, head, tail):
    rs.set_counters(head, tail)
    mo.head[:len(head)], mo.tail[:len(tail)] = list(head), list(tail)


def set_free(rs, mo, e, free):
    """the head alone, through usn_ringset_set_head: receiver e has `free` slots left"""
    mo.head[e] = (mo.tail[e] - (int(mo.size[e]) - free)) & M32
    rs.set_head(mo.head[:e + 1])


def append_and_check(ctx, s, rs, mo, rings, regs, pipe0=False):
    ctx.deliver_rings([g[0] for g in rings], [g[1] for g in rings], rs, s)
    hdr = rs.info(s, strict=False)
    x = mo.append(rings, regs, pipe0)
    print("offered %d accepted %d dropped %d flags %d; receiver 1: first %d acc %d drop %d seg_acc %s" % (
        hdr.offered, hdr.accepted, hdr.dropped, hdr.flags, rs.first()[1], rs.acc()[1], rs.drop()[1], rs.seg_acc()[1]))
    assert (hdr.offered, hdr.accepted, hdr.dropped) == (x["offered"], x["acc"].sum(), x["drop"].sum())
    assert (hdr.n_recv, hdr.flags) == ((x["acc"] > 0).sum(), x["flags"])
    assert hdr.status == (lib.USN_ERANGE if x["flags"] else 0)
    for f in ("first", "acc", "drop", "seg_acc"):
        np.testing.assert_array_equal(getattr(rs, f)(), x[f], f)
    np.testing.assert_array_equal(rs.tail(), mo.tail)
    np.testing.assert_array_equal(rs.head(), mo.head)
    np.testing.assert_array_equal(rs.lens(), mo.lens)
    np.testing.assert_array_equal(rs.src(), mo.src)
    np.testing.assert_array_equal(rs.slots(), mo.frames)
    return x


@pytest.fixture(scope="module")
def round3():
    """test_tile_across_segment_ends' round: receiver 1's tile 1 holds the end of ring 0, all of 1, the start of 2"""
    ctx, s, regs = make_ctx()
    rings = [add_ring(ctx, s, base.rx_kinds(1023)),
             add_ring(ctx, s, [ARP, EP + 1, EAPOL, NIC, EP + 3, ARP, DROP], src=2),
             add_ring(ctx, s, base.rx_kinds(2 * P + 5))]
    yield ctx, s, regs, rings, reference(rings, regs, False)[1]
    ctx.close()


@pytest.mark.parametrize("count", [1, 3])
def test_ample_rings_equal_the_round_delivery(round3, count):
    ctx, s, regs, rings, _ = round3
    rings = rings[:count] if count > 1 else [add_ring(ctx, s, base.rx_kinds(1025))]
    rs, mo = new_set(ctx, [512, 2048, 512, 512, 512])
    x = append_and_check(ctx, s, rs, mo, rings, regs)
    assert x["flags"] == 0 and x["acc"][1] > (2 * P if count > 1 else P)
    rv = lib.DeviceRoundDelivery(ctx, x["offered"], 64, poison=POISON)
    ctx.deliver_round([g[0] for g in rings], [g[1] for g in rings], rv, s)
    rv.info(s)
    for e in regs:
        src, lens, slots, _ = rv.ring(e)
        for got, want in zip(rs.ring(e), (lens, src, slots)):
            np.testing.assert_array_equal(got, want)
    rv.free()
    rs.free()


@pytest.mark.parametrize("a", [700, 512, 1023, 1024 - 16])
def test_wrap(a):
    """ring 1 (1024 slots) takes a frames, is drained, and takes about 700 more across its end: off
    any 16-slot boundary, on a tile start, one slot before the end, 16 before it; a third call
    without a drain meets the partly full ring"""
    ctx, s, regs = make_ctx()
    rs, mo = new_set(ctx, [256, 1024, 256, 256, 256])
    fill, more = add_ring(ctx, s, [EP + 1] * a), add_ring(ctx, s, base.rx_kinds(1025))
    assert append_and_check(ctx, s, rs, mo, [fill], regs)["acc"][1] == a
    mo.head = list(mo.tail)
    rs.set_head(mo.head[:5], s)
    x = append_and_check(ctx, s, rs, mo, [more], regs)
    took = x["acc"][1]
    assert x["flags"] == 0 and 600 < took and a + took > 1024
    x = append_and_check(ctx, s, rs, mo, [more], regs)
    assert x["flags"] == lib.DV_DROPPED and x["acc"][1] == 1024 - took > 0
    ctx.close()


@pytest.mark.parametrize("where", ["none", "one", "segment0", "segment0+1", "inside2", "all", "all-1"])
def test_tail_drop_position(round3, where):
    ctx, s, regs, rings, seg = round3
    offered = int(seg[1].sum())
    free = {"none": 0, "one": 1, "segment0": seg[1, 0], "segment0+1": seg[1, 0] + 1,
            "inside2": seg[1, 0] + seg[1, 1] + P + 37, "all": offered, "all-1": offered - 1}[where]
    assert where != "inside2" or (free % P != 0 and free < offered)
    rs, mo = new_set(ctx, [512, 2048, 512, 512, 512])
    set_free(rs, mo, 1, int(free))
    x = append_and_check(ctx, s, rs, mo, rings, regs)
    assert x["acc"][1] == free and x["flags"] == (0 if where == "all" else lib.DV_DROPPED)
    rs.free()


def test_truncated_three_list_segment():
    """test_three_list_cut_at_an_unaligned_position's round sent by pipe 3: receiver 0's room ends
    inside segment 1 past its first tile, so the last tile merges own + NIC + FLOOD and is cut short"""
    ctx, s, regs = make_ctx(pipe0=True)
    side = [[EP + 0, EP + 1, ARP, EP + 0, EP + 3][i % 5] for i in range(300)]
    rings = [add_ring(ctx, s, side, src=3), add_ring(ctx, s, [TX_CYCLE[i % 7] for i in range(2 * P + 3)], src=2),
             add_ring(ctx, s, side, src=3)]
    seg = reference(rings, regs, True)[1]
    rs, mo = new_set(ctx, [1024, 512, 512, 512, 512, 0, 512])
    set_free(rs, mo, 0, int(seg[0, 0]) + P + 77)
    x = append_and_check(ctx, s, rs, mo, rings, regs, pipe0=True)
    assert 0 < seg[0, 0] < P and x["seg_acc"][0].tolist()[:3] == [seg[0, 0], P + 77, 0] and seg[0, 1] > P + 77
    ctx.close()


@pytest.mark.parametrize("big", [False, True])
def test_tiny_and_absent_rings(big):
    """rings of 1, 2 and 8 slots, and none at all for the registered receiver 4"""
    ctx, s, regs = make_ctx()
    kinds = [[EP + 1], [ARP, EP + 3], [EP + 2, EP + 2, DROP], [NIC], [ARP], [EP + 1, EAPOL, NIC], [DROP], [EP + 4, ARP]]
    rings = [add_ring(ctx, s, base.rx_kinds(1025))] if big else \
        [add_ring(ctx, s, k, src=2 * (i % 2)) for i, k in enumerate(kinds)]
    rs, mo = new_set(ctx, [64, 1, 2, 8, 0])
    x = append_and_check(ctx, s, rs, mo, rings, regs)
    assert x["acc"][1:5].tolist() == [1, 2, 8 if big else 5, 0] and x["drop"][4] > 0
    x = append_and_check(ctx, s, rs, mo, rings, regs)   # full now
    assert x["acc"][1:5].tolist() == [0, 0, 0 if big else 3, 0]
    ctx.close()


@pytest.mark.parametrize("slot,drop_long", [(1536, False), (128, False), (128, True)])
def test_layouts_and_long_frames(slot, drop_long):
    """test_mixed_layouts' rings; drop_long: every receiver's room ends before its first frame longer
    than the slot, so no accepted frame is long and USN_DV_LONG stays clear"""
    ctx, s, regs = make_ctx()
    rng = np.random.default_rng(7)
    pool = np.array([14, 15, 16, 17, 31, 32, 33, 60, 64, 65, 127, 128])
    rings = [add_ring(ctx, s, base.rx_kinds(200)),
             add_ring(ctx, s, [EP + 1 + i % 4 if i % 3 else ARP for i in range(300)], stride=128,
                      lens=pool[rng.integers(0, pool.size, 300)], poison_in=True),
             add_ring(ctx, s, [EP + 1 + i % 4 if i % 5 else EAPOL for i in range(100)], offsets=True,
                      lens=np.array([60, 1024, 1025, 1514])[rng.integers(0, 4, 100)])]
    rs, mo = new_set(ctx, [512] * 5, slot)
    if drop_long:
        want, seg = reference(rings, regs, False)
        for e in regs:
            long_at = np.flatnonzero(rings[2][3][want[2][e]] > slot)
            if long_at.size:
                set_free(rs, mo, e, int(seg[e, 0] + seg[e, 1] + long_at[0]))
    x = append_and_check(ctx, s, rs, mo, rings, regs)
    assert x["flags"] == (lib.DV_DROPPED if drop_long else lib.DV_LONG if slot == 128 else 0)
    ctx.close()


@pytest.mark.parametrize("ahead", [False, True])
def test_counters(ahead):
    """head = tail = 2^32 - 300: the append crosses the 32-bit wrap of the counters; a head ahead
    of the tail leaves no room"""
    ctx, s, regs = make_ctx()
    rs, mo = new_set(ctx, [256, 1024, 256, 256, 256])
    tail = [(1 << 32) - 300] * 5
    set_counters(rs, mo, [t + 5 & M32 for t in tail] if ahead else tail, tail)
    x = append_and_check(ctx, s, rs, mo, [add_ring(ctx, s, base.rx_kinds(1025))], regs)
    assert x["acc"].sum() == 0 if ahead else (x["flags"] == 0 and mo.tail[1] < 1024 and x["acc"][1] > 600)
    ctx.close()


def test_unfinalized_tx_ring_is_busy():
    ctx, s, regs = make_ctx()
    rings = [add_ring(ctx, s, base.rx_kinds(100)),
             add_ring(ctx, s, [TX_CYCLE[i % 7] for i in range(50)], src=2, finalize=False)]
    rs, mo = new_set(ctx, [128] * 5)
    with pytest.raises(lib.UsnError, match="EBUSY"):
        ctx.deliver_rings([g[0] for g in rings], [g[1] for g in rings], rs, s)
    ctx.finalize(rings[1][0], rings[1][1], s)
    append_and_check(ctx, s, rs, mo, rings, regs)
    ctx.close()
