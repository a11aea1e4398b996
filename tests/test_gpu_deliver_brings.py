"""usn_deliver_brings: a poll round appended to persistent byte-compact rings, bit-exact
against a plain model: per registered receiver test_gpu_deliver_round.reference(...) over
the rings in order, the frames written one by one into numpy descriptor and byte rings;
a frame is taken while a descriptor and its 16-byte units are free, and the first that
finds neither ends the receiver's run.  After every call first, bfirst, acc, drop,
acc_units, seg_acc, head, tail, btail and the header are compared, and lens / src /
pos16 / frames as WHOLE arrays against the model, which starts from the poison.
"""
import numpy as np
import pytest

from usnetd_amd import lib
import test_gpu_deliver as base
from test_gpu_deliver import ARP, DROP, EAPOL, EP, NIC, P, POISON
from test_gpu_deliver_packed import pool_lens
from test_gpu_deliver_round import TX_CYCLE, add_ring, make_ctx, reference

pytestmark = pytest.mark.gpu
RM, IDS, M32 = lib.USN_ROUND_MAX, lib.USN_MAX_ENDPOINTS + 1, 0xFFFFFFFF
C3 = np.array([64, 64, 64, 64, 64, 64, 64, 576, 576, 576, 576, 1500, 60, 1499])   # c3's 7 : 4 : 1, and two odd ones


def units(ln):
    return np.maximum(1, (np.asarray(ln, np.int64) + 15) // 16)


def mixed_ring(ctx, s, kinds, seed, **kw):
    return add_ring(ctx, s, kinds, stride=2048, lens=C3[np.random.default_rng(seed).integers(0, C3.size, len(kinds))], **kw)


def unit_ring(ctx, s, n, src=0):
    """n flooded 16-byte frames: one unit each, the way the tests place a ring's counters"""
    return add_ring(ctx, s, [ARP] * n, src=src, lens=[16] * n)


class Model:
    def __init__(self, D, B):
        self.D, self.B = np.zeros(IDS, np.int64), np.zeros(IDS, np.int64)
        self.D[:len(D)], self.B[:len(B)] = D, B
        self.doff, self.uoff = np.concatenate([[0], np.cumsum(self.D)]), np.concatenate([[0], np.cumsum(self.B)])
        self.head, self.tail, self.btail = [0] * IDS, [0] * IDS, [0] * IDS
        nd, nu = max(int(self.doff[-1]), 1), max(int(self.uoff[-1]), 1)
        self.lens = np.full(nd, POISON * 0x0101, np.uint16)
        self.src, self.pos16 = np.full(nd, POISON * 0x01010101, np.uint32), np.full(nd, POISON * 0x01010101, np.uint32)
        self.frames = np.full((nu, 16), POISON, np.uint8)

    def free(self, e):
        D, B = int(self.D[e]), int(self.B[e])
        if D == 0:
            return 0, 0
        fill = (self.tail[e] - self.head[e]) & M32
        used = (self.btail[e] - int(self.pos16[self.doff[e] + (self.head[e] & (D - 1))])) & M32 if fill else 0
        return D - min(fill, D), B - min(used, B)

    def append(self, rings, regs, pipe0):
        want, _ = reference(rings, regs, pipe0)
        first, bfirst = np.array(self.tail), np.array(self.btail)
        seg_acc, offered, acc_units = np.zeros((IDS, RM), np.int64), np.zeros(IDS, np.int64), np.zeros(IDS, np.int64)
        for e in regs:
            (free_d, free_u), D, B, j, cum, taking = self.free(e), int(self.D[e]), int(self.B[e]), 0, 0, True
            for k, (_, _, F, lens, starts, _) in enumerate(rings):
                for i in want[k][e]:
                    offered[e] += 1
                    ln, u = int(lens[i]), int(units(lens[i]))
                    taking = taking and j < free_d and cum + u <= free_u   # one cut: nothing behind a dropped frame
                    if not taking:
                        continue
                    q, pos = int(self.doff[e]) + ((first[e] + j) & (D - 1)), (int(bfirst[e]) + cum) & M32
                    body = np.zeros(16 * u, np.uint8)
                    body[:ln] = F[int(starts[i]):int(starts[i]) + ln]
                    self.frames[int(self.uoff[e]) + ((pos + np.arange(u)) & (B - 1))] = body.reshape(u, 16)
                    self.lens[q], self.src[q], self.pos16[q] = ln, i, pos
                    j, cum = j + 1, cum + u
                    seg_acc[e, k] += 1
            self.tail[e], self.btail[e], acc_units[e] = (self.tail[e] + j) & M32, (self.btail[e] + cum) & M32, cum
        acc = seg_acc.sum(1)
        return dict(first=first, bfirst=bfirst, seg_acc=seg_acc, acc=acc, drop=offered - acc, acc_units=acc_units,
                    offered=int(offered.sum()), flags=lib.DV_DROPPED if (offered > acc).any() else 0)


def new_set(ctx, D, B):
    return lib.DeviceBRingSet(ctx, D, B, poison=POISON), Model(D, B)


def set_counters(rs, mo, head, tail, btail):
    rs.set_counters(head, tail, btail)
    mo.head[:len(head)], mo.tail[:len(tail)], mo.btail[:len(btail)] = list(head), list(tail), list(btail)


def set_head(rs, mo, e, h):
    mo.head[e] = h & M32
    rs.set_head(mo.head[:e + 1])


def append_and_check(ctx, s, rs, mo, rings, regs, pipe0=False):
    ctx.deliver_brings([g[0] for g in rings], [g[1] for g in rings], rs, s)
    hdr = rs.info(s, strict=False)
    x = mo.append(rings, regs, pipe0)
    e = 0 if pipe0 else 1
    print("offered %d accepted %d (%d units) dropped %d flags %d; receiver %d: first %d bfirst %d acc %d units %d seg_acc %s" % (
        hdr.offered, hdr.accepted, hdr.accepted_units, hdr.dropped, hdr.flags, e, rs.first()[e], rs.bfirst()[e],
        rs.acc()[e], rs.acc_units()[e], rs.seg_acc()[e]))
    assert (hdr.offered, hdr.accepted, hdr.dropped) == (x["offered"], x["acc"].sum(), x["drop"].sum())
    assert (hdr.accepted_units, hdr.n_recv, hdr.flags) == (x["acc_units"].sum(), (x["acc"] > 0).sum(), x["flags"])
    assert hdr.status == (lib.USN_ERANGE if x["flags"] else 0)
    for f in ("first", "bfirst", "acc", "drop", "acc_units", "seg_acc"):
        np.testing.assert_array_equal(getattr(rs, f)(), x[f], f)
    for f in ("head", "tail", "btail", "lens", "src", "pos16"):
        np.testing.assert_array_equal(getattr(rs, f)(), getattr(mo, f), f)
    np.testing.assert_array_equal(rs.units(), mo.frames)
    return x


@pytest.fixture(scope="module")
def round3():
    """the ring tests' round with mixed lengths: receiver 1's tile 1 holds the end of ring 0, all of 1, the start
    of 2; `ones` floods 32768 one-unit frames, which fill a byte ring so that the head alone sets free_u"""
    ctx, s, regs = make_ctx()
    kinds0 = base.rx_kinds(1023)
    rings = [add_ring(ctx, s, kinds0, stride=2048, lens=np.r_[1500, C3[np.random.default_rng(1).integers(0, C3.size, 1022)]]),
             add_ring(ctx, s, [ARP, EP + 1, EAPOL, NIC, EP + 3, ARP, DROP], src=2),
             mixed_ring(ctx, s, base.rx_kinds(2 * P + 5), 2)]
    want, seg = reference(rings, regs, False)
    u1 = np.concatenate([units(rings[k][3][want[k][1]]) for k in range(3)])   # receiver 1's round ring, in units
    yield ctx, s, regs, rings, seg, u1, unit_ring(ctx, s, 32768)
    ctx.close()


@pytest.mark.parametrize("count", [1, 3])
def test_ample_rings_equal_the_round_delivery(round3, count):
    ctx, s, regs, rings = round3[:4]
    rings = rings[:count] if count > 1 else [mixed_ring(ctx, s, base.rx_kinds(1025), 3)]
    rs, mo = new_set(ctx, [512, 4096, 512, 512, 512], [32768, 131072, 32768, 32768, 32768])
    x = append_and_check(ctx, s, rs, mo, rings, regs)
    assert x["flags"] == 0 and x["acc"][1] > (2 * P if count > 1 else P)
    rv = lib.DeviceRoundDelivery(ctx, x["offered"], 2048, poison=POISON)
    ctx.deliver_round([g[0] for g in rings], [g[1] for g in rings], rv, s)
    rv.info(s)
    for e in regs:
        src, lens, slots, _ = rv.ring(e)
        got = rs.ring(e)
        np.testing.assert_array_equal(got[0], lens)
        np.testing.assert_array_equal(got[1], src)
        assert len(got[2]) == lens.size and all(np.array_equal(b, sl[:b.size]) and b.size == 16 * units(ln)
                                                for b, sl, ln in zip(got[2], slots, lens))
    rv.free()
    rs.free()


@pytest.mark.parametrize("where", ["first", "boundary", "boundary-1", "later", "segment", "descriptors", "nothing"])
def test_the_cut(round3, where):
    """descriptors ample and free_u set through the head: the byte ring is filled by one-unit frames and
    head = h frees exactly h units.  `frames` of receiver 1's round fit, the next one lacks a unit (where
    it has more than one); descriptors: the reverse, the byte ring ample and h descriptors free"""
    ctx, s, regs, rings, seg, u1, ones = round3
    frames = {"first": 100, "boundary": P, "boundary-1": P - 1, "later": P + 37, "segment": int(seg[1, 0]) + 2,
              "descriptors": P + 37, "nothing": 0}[where]
    cum = int(u1[:frames].sum())
    h = {"boundary": cum, "descriptors": frames, "nothing": 3}.get(where, cum + int(u1[frames]) - 1)
    by_desc = where == "descriptors"
    rs, mo = new_set(ctx, [0, 1024 if by_desc else 65536], [0, 65536 if by_desc else 32768])
    filled = append_and_check(ctx, s, rs, mo, [ones], regs)
    assert filled["acc"][1] == (1024 if by_desc else 32768) and u1[0] > 3 and u1[P - 1] > 1
    set_head(rs, mo, 1, int(h))
    x = append_and_check(ctx, s, rs, mo, rings, regs)
    assert x["acc"][1] == frames and x["flags"] == lib.DV_DROPPED
    assert by_desc or x["acc_units"][1] == cum <= h < cum + u1[frames]
    if where == "segment":
        assert x["seg_acc"][1].tolist()[:3] == [seg[1, 0], 2, 0] and seg[1, 1] > 2 and seg[1, 2] > 0
    rs.free()


def test_the_cut_inside_a_three_way_merge():
    """the ring tests' truncated three-list segment: receiver 0's units end inside segment 1 past its
    first tile, where own + NIC + FLOOD merge"""
    ctx, s, regs = make_ctx(pipe0=True)
    side = [[EP + 0, EP + 1, ARP, EP + 0, EP + 3][i % 5] for i in range(300)]
    rings = [add_ring(ctx, s, side, src=3), mixed_ring(ctx, s, [TX_CYCLE[i % 7] for i in range(2 * P + 3)], 4, src=2),
             add_ring(ctx, s, side, src=3)]
    want, seg = reference(rings, regs, True)
    u0 = np.concatenate([units(rings[k][3][want[k][0]]) for k in range(3)])
    frames = int(seg[0, 0]) + P + 77
    rs, mo = new_set(ctx, [65536], [32768])
    append_and_check(ctx, s, rs, mo, [unit_ring(ctx, s, 32768, src=3)], regs, pipe0=True)
    set_head(rs, mo, 0, int(u0[:frames].sum()))
    x = append_and_check(ctx, s, rs, mo, rings, regs, pipe0=True)
    assert 0 < seg[0, 0] < P and x["seg_acc"][0].tolist()[:3] == [seg[0, 0], P + 77, 0] and seg[0, 1] > P + 77
    ctx.close()


@pytest.mark.parametrize("where", ["inside a 1500-byte frame", "tile start", "one unit before the end"])
def test_wrap(where):
    """a fill, the consumer takes all of it, and about 700 mixed frames cross the end of the byte ring
    (32768 units) and, elsewhere, of the descriptor ring (1024); a third call without a head move meets
    the partly full ring"""
    ctx, s, regs = make_ctx()
    D, B = 1024, 32768
    rs, mo = new_set(ctx, [64, D, 64, 64, 64], [256, B, 256, 256, 256])
    more = add_ring(ctx, s, base.rx_kinds(1025), stride=2048,
                    lens=np.r_[1500, C3[np.random.default_rng(5).integers(0, C3.size, 1024)]])
    u1 = units(more[3][reference([more], regs, False)[0][0][1]])
    assert append_and_check(ctx, s, rs, mo, [add_ring(ctx, s, [EP + 1] * 100)], regs)["acc"][1] == 100
    j = int(np.flatnonzero(u1[300:] == 94)[0]) + 300   # a 1500-byte frame
    tail, btail = {"inside a 1500-byte frame": (1000, B - int(u1[:j].sum()) - 40), "tile start": (D - P, B - int(u1[:P].sum())),
                   "one unit before the end": (D - 1, B - 1)}[where]
    set_counters(rs, mo, [0, tail], [0, tail], [0, btail])   # empty, at these positions
    x = append_and_check(ctx, s, rs, mo, [more], regs)
    took = x["acc"][1]
    assert took == u1.size > 600 and btail + x["acc_units"][1] > B and tail + took > D
    x = append_and_check(ctx, s, rs, mo, [more], regs)
    assert x["flags"] == lib.DV_DROPPED and 0 < x["acc"][1] <= D - took
    ctx.close()


@pytest.mark.parametrize("how", ["full", "head ahead", "used > B"])
def test_nothing_free(how):
    """ids 1 and 2: a full ring, a head ahead of the tail, more units in use than the ring has; id 3 has a ring
    and a bin but is no longer registered; id 4 is registered without a ring.  Everything is dropped"""
    ctx, s, regs = make_ctx()
    rs, mo = new_set(ctx, [0, 64, 64, 64, 0], [0, 64, 64, 64, 0])
    ring = mixed_ring(ctx, s, base.rx_kinds(300), 6)
    if how != "head ahead":
        n = 64 if how == "full" else 10
        assert append_and_check(ctx, s, rs, mo, [unit_ring(ctx, s, n)], regs)["acc"][1:4].tolist() == [n] * 3
    ctx.endpoint_remove(3)
    regs = [0, 1, 2, 4]
    if how == "head ahead":
        set_counters(rs, mo, [0, 5, 5, 5], [0] * 4, [0] * 4)
    elif how == "used > B":
        set_counters(rs, mo, [0] * 4, [0, 10, 10, 10], [0, 81, 81, 81])
    before = list(mo.tail), list(mo.btail)
    x = append_and_check(ctx, s, rs, mo, [ring], regs)
    assert x["acc"].sum() == 0 and x["flags"] == lib.DV_DROPPED and (x["drop"][[1, 2, 4]] > 0).all() and x["drop"][3] == 0
    assert (mo.tail, mo.btail) == before and (ring[1].decisions() & 0xFFFF == 3).any()
    ctx.close()


def test_more_tiles_than_one_scan_block():
    """the packed test's 1100 more pipes, each with a one-tile ring of the flooded frames: every tile is a run's first"""
    ctx, s, _ = make_ctx()
    n = 40
    ring = add_ring(ctx, s, np.where(np.arange(n) % 8 == 0, ARP, EP + 1 + np.arange(n) % 4), stride=2048, lens=pool_lens(n, 6))
    for e in range(5, 1105):
        ctx.endpoint_add(e, lib.EP_PIPE, 0)
    rs, mo = new_set(ctx, [32] * 1105, [1024] * 1105)
    x = append_and_check(ctx, s, rs, mo, [ring], list(range(1105)))
    assert (x["acc"] > 0).sum() > 1024 and x["acc"][1104] >= 5
    ctx.close()


@pytest.mark.parametrize("length", [64, 60])
def test_uniform_fast_path(length):
    """every tile has one unit count: 64 exactly, and 60 with its masked tail"""
    ctx, s, regs = make_ctx()
    ring = add_ring(ctx, s, base.rx_kinds(1025), lens=np.full(1025, length), poison_in=True)
    rs, mo = new_set(ctx, [64, 1024, 256, 256, 256], [256, 4096, 1024, 1024, 1024])
    x = append_and_check(ctx, s, rs, mo, [ring], regs)
    assert x["flags"] == 0 and x["acc"][1] > P and x["acc_units"][1] == 4 * x["acc"][1]
    ctx.close()
