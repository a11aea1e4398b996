"""usn_brings_drain: the byte rings' queued frames gathered unit for unit, bit-exact against
plain numpy over the set AS FOUND: head, tail, btail, lens, src, pos16 and the units are read
back before the call and the expectation is the contract of usn_classify.h "byte-ring
drain" over them alone (int64, & 0xFFFFFFFF), so nothing here leans on the appends being
right.  Every output is compared as a WHOLE array (poison outside the selection), then the
per-id arrays, the header and status, head after the call, and that the set did not change.
"""
import numpy as np
import pytest

from usnetd_amd import lib
import test_gpu_deliver as base
from test_gpu_deliver import ARP, EP, P, POISON
from test_gpu_deliver_brings import C3, mixed_ring, units
from test_gpu_deliver_packed import pool_lens
from test_gpu_deliver_round import add_ring, make_ctx, reference

pytestmark = pytest.mark.gpu
IDS, M32, UT, ALL = lib.USN_MAX_ENDPOINTS + 1, 0xFFFFFFFF, lib.USN_BDRAIN_UTILE, [0xFFFFFFFF] * 5
FIELDS = ("head", "tail", "btail", "lens", "src", "pos16", "units")
P16, P32 = POISON * 0x0101, POISON * 0x01010101


def ring_state(rs):
    st = {k: getattr(rs, k)() for k in FIELDS}
    st.update({k: st[k].astype(np.int64) for k in FIELDS[:3]})
    return st


def expect(rs, st, budget, cap):
    """the contract over the state st"""
    D, B, doff, uoff, bud = (np.zeros(IDS, np.int64) for _ in range(5))
    D[:rs.doff.size - 1], B[:rs.uoff.size - 1] = np.diff(rs.doff), np.diff(rs.uoff)
    doff[:rs.doff.size - 1], uoff[:rs.uoff.size - 1], bud[:len(budget)] = rs.doff[:-1], rs.uoff[:-1], budget
    has, pos = D > 0, st["pos16"].astype(np.int64)
    h, btail = st["head"], st["btail"]
    f = (st["tail"] - h) & M32
    p0 = np.where(has, pos[np.where(has, doff + (h & (D - 1)), 0)], 0)
    used = np.where(f > 0, (btail - p0) & M32, 0)
    sound = (f <= D) & (f <= used) & (used <= B)
    avail = np.where(sound, f, 0)
    ep_off = np.minimum(np.concatenate([[0], np.cumsum(np.minimum(avail, bud))]), cap)
    take = np.diff(ep_off)
    p1 = np.where(take == avail, btail, pos[np.where(has, doff + ((h + take) & (D - 1)), 0)])
    nu = np.where(take > 0, (p1 - p0) & M32, 0)
    bad = bool(((take > 0) & (take < avail) & ((nu < take) | (nu > used))).any())
    nu = np.minimum(nu, B)
    boff = 16 * np.concatenate([[0], np.cumsum(nu)])
    q, off16, body = [np.empty(0, np.int64)], [np.empty(0, np.int64)], [np.empty(0, np.uint8)]
    for e in np.flatnonzero(take):
        qe = doff[e] + ((h[e] + np.arange(take[e])) & (D[e] - 1))
        bad |= bool((np.r_[pos[qe][1:], p1[e]] != ((pos[qe] + units(st["lens"][qe])) & M32)).any())   # the chain
        q.append(qe)
        off16.append(boff[e] // 16 + np.minimum((pos[qe] - p0[e]) & M32, nu[e]))
        body.append(st["units"][uoff[e] + ((p0[e] + np.arange(nu[e])) & (B[e] - 1))].reshape(-1))
    flags = (lib.DR_MORE if (avail > take).any() else 0) | (lib.DR_BADCOUNT if (has & (f != 0) & ~sound).any() else 0) \
        | (lib.DR_BADDESC if bad else 0)
    return dict(take=take, left=avail - take, ep_off=ep_off, boff=boff, need=int(boff[-1]), flags=flags, nu=nu,
                q=np.concatenate(q), off16=np.concatenate(off16), body=np.concatenate(body))


def drain_and_check(ctx, s, rs, budget=ALL, cap=None, cap_bytes=None):
    cap = rs.total_desc if cap is None else cap
    cap_bytes = 16 * rs.total_units if cap_bytes is None else cap_bytes
    st = ring_state(rs)
    x = expect(rs, st, budget, cap)
    fits, sel = x["need"] <= cap_bytes, x["q"].size
    flags = x["flags"] | (0 if fits else lib.DV_OVERFLOW_BYTES)
    moved = fits and not flags & lib.DR_BADDESC
    dr = lib.DeviceDrain(ctx, cap, cap_bytes, poison=POISON)
    dr.set_budget(budget, s)
    ctx.drain_brings(rs, dr, s)
    hdr = dr.info(s, strict=False, brings=True)
    assert (hdr.need_bytes, hdr.cap_bytes, hdr.selected, hdr.taken) == (x["need"], cap_bytes, sel, sel if moved else 0)
    assert (hdr.n_recv, hdr.flags) == ((x["take"] > 0).sum(), flags)
    assert hdr.status == (lib.USN_ERANGE if flags & (lib.DV_OVERFLOW_BYTES | lib.DR_BADCOUNT | lib.DR_BADDESC) else 0)
    for got, want in ((dr.from_(), st["head"]), (dr.take(), x["take"]), (dr.left(), x["left"]), (dr.ep_off(), x["ep_off"]),
                      (dr.ep_boff(), x["boff"])):
        np.testing.assert_array_equal(got, want)
    want = np.full(cap_bytes, POISON, np.uint8)
    if flags & lib.DR_BADDESC:   # unspecified inside [0, min(need_bytes, cap_bytes)) and [0, selected)
        end = min(x["need"], cap_bytes)
        np.testing.assert_array_equal(dr.bytes()[end:], want[end:])
        np.testing.assert_array_equal(dr.off16()[sel:], np.full(cap - sel, P32, np.uint32))
    else:
        if fits:
            want[:x["need"]] = x["body"]
        np.testing.assert_array_equal(dr.bytes(), want)
    for got, val, fill in ((dr.lens(), st["lens"][x["q"]], P16), (dr.src(), st["src"][x["q"]], P32),
                           (dr.off16(), x["off16"], P32))[:2 if flags & lib.DR_BADDESC else 3]:
        want = np.full(cap, fill, got.dtype)
        want[:sel] = val
        np.testing.assert_array_equal(got, want)
    after = ring_state(rs)
    np.testing.assert_array_equal(after.pop("head"), (st.pop("head") + (x["take"] if moved else 0)) & M32)
    for k in st:
        np.testing.assert_array_equal(after[k], st[k], k)
    dr.free()
    return x


def append(ctx, s, rs, rings):
    ctx.deliver_brings([g[0] for g in rings], [g[1] for g in rings], rs, s)
    return rs.info(s, strict=False)


def upload(rs, field, values):
    rs.buf.upload(np.ascontiguousarray(values), offset=getattr(rs.desc, field) - rs.buf.ptr)


@pytest.fixture(scope="module")
def rounds():
    """the byte-ring tests' three-ring mixed round, one ring of about as many frames, and one of 1025 plain ones"""
    ctx, s, regs = make_ctx()
    three = [mixed_ring(ctx, s, base.rx_kinds(1023), 1), add_ring(ctx, s, [ARP, EP + 1, ARP, EP + 3, ARP], src=2),
             mixed_ring(ctx, s, base.rx_kinds(2 * P + 5), 2)]
    yield ctx, s, {1: [mixed_ring(ctx, s, base.rx_kinds(2500), 3)], 3: three, 0: [add_ring(ctx, s, base.rx_kinds(1025))]}
    ctx.close()


def ample(ctx):
    return lib.DeviceBRingSet(ctx, [512, 4096, 512, 512, 512], [32768, 131072, 32768, 32768, 32768], poison=POISON)


@pytest.mark.parametrize("count", [1, 3])
def test_tiles(rounds, count):
    ctx, s, rings = rounds
    rs = ample(ctx)
    assert append(ctx, s, rs, rings[count]).flags == 0
    x = drain_and_check(ctx, s, rs)
    assert x["flags"] == 0 and x["take"][1] > 2 * P and x["nu"][1] > 2 * UT and (x["take"][2:5] > 0).all()
    assert drain_and_check(ctx, s, rs)["q"].size == 0   # everything is empty now: nothing is written
    rs.free()


@pytest.mark.parametrize("where", ["inside a 1500-byte frame", "unit-tile start", "one unit before the end"])
def test_wrap(where):
    """the empty ring 1 placed so that about 700 mixed frames cross the end of its unit ring (32768) and, at
    another frame, of its descriptor ring (1024); drained, appended to again, drained again"""
    ctx, s, regs = make_ctx()
    D, B = 1024, 32768
    rs = lib.DeviceBRingSet(ctx, [64, D, 64, 64, 64], [256, B, 256, 256, 256], poison=POISON)
    more = add_ring(ctx, s, base.rx_kinds(1025), stride=2048,
                    lens=np.r_[1500, C3[np.random.default_rng(5).integers(0, C3.size, 1024)]])
    u1 = units(more[3][reference([more], regs, False)[0][0][1]])
    j = int(np.flatnonzero(u1[300:] == 94)[0]) + 300   # a 1500-byte frame
    tail, btail = {"inside a 1500-byte frame": (1000, B - int(u1[:j].sum()) - 40), "unit-tile start": (D - P, B - UT),
                   "one unit before the end": (D - 1, B - 1)}[where]
    rs.set_counters([0, tail], [0, tail], [0, btail])   # empty, at these positions
    for _ in range(2):   # the second append lands only because the drain moved the head
        append(ctx, s, rs, [more])   # the small rings drop some; ring 1 takes all
        x = drain_and_check(ctx, s, rs)
        assert x["take"][1] == u1.size > 600 and x["nu"][1] == u1.sum() > UT
    assert tail + u1.size > D and btail + u1.sum() > B
    ctx.close()


@pytest.mark.parametrize("how", ["b0", "b1", "bP", "bP+37", "ball", "cap_in_1", "cap_at_1_end", "cap_in_0"])
def test_budget_and_cap(rounds, how):
    ctx, s, rings = rounds
    rs = ample(ctx)
    append(ctx, s, rs, rings[3])
    n0, n1 = (int(v) for v in rs.tail()[:2])
    assert n0 >= 2 and n1 > 2 * P
    b1 = {"b0": 0, "b1": 1, "bP": P, "bP+37": P + 37}.get(how, M32)
    cap = {"cap_in_1": n0 + P + 37, "cap_at_1_end": n0 + n1, "cap_in_0": n0 - 1}.get(how)
    x = drain_and_check(ctx, s, rs, [M32, b1, M32, M32, M32], cap)
    assert x["take"][1] == {"cap_in_1": P + 37, "cap_in_0": 0}.get(how, min(b1, n1))
    assert bool(x["flags"] & lib.DR_MORE) == (how not in ("ball",)) and x["take"].sum() == (cap or x["take"].sum())
    y = drain_and_check(ctx, s, rs)   # the rest, in order
    np.testing.assert_array_equal(y["take"], x["left"])
    assert y["flags"] == 0
    rs.free()


@pytest.mark.parametrize("delta", [-16, 0])
def test_byte_overflow(rounds, delta):
    ctx, s, rings = rounds
    rs = ample(ctx)
    append(ctx, s, rs, rings[3])
    need = expect(rs, ring_state(rs), ALL, rs.total_desc)["need"]
    drain_and_check(ctx, s, rs, cap_bytes=need + delta)   # -16: nothing moves; 0: fits, poison from need_bytes on
    if delta:
        assert drain_and_check(ctx, s, rs, cap_bytes=need)["need"] == need   # still all there
    rs.free()


@pytest.mark.parametrize("kind", ["wrap32", "ahead", "used>B", "used<fill", "handmade"])
def test_counters(rounds, kind):
    """counters across 2^32; corrupt counters of ring 1 (skipped, the others drained); a hand-made ring of lens
    0 .. 70 over poisoned units: they arrive verbatim and a zero-length frame keeps its unit"""
    ctx, s, rings = rounds
    D, B, t0 = 1024, 32768, (1 << 32) - 300
    rs = lib.DeviceBRingSet(ctx, [256, D, 256, 256, 256], [8192, B, 8192, 8192, 8192], poison=POISON)
    if kind == "handmade":
        n, h = 600, 900
        q = 256 + ((h + np.arange(n)) & (D - 1))
        lens, pos = rs.lens(), rs.pos16()
        lens[q] = np.arange(n) % 71
        pos[q] = (t0 + np.r_[0, np.cumsum(units(lens[q]))[:-1]]) & M32
        upload(rs, "lens", lens), upload(rs, "pos16", pos)
        rs.set_counters([0, h], [0, h + n], [0, (t0 + int(units(lens[q]).sum())) & M32])
        x = drain_and_check(ctx, s, rs)
        assert x["flags"] == 0 and x["take"][1] == n and x["nu"][1] == units(lens[q]).sum() > n
        return rs.free()
    if kind == "wrap32":
        rs.set_counters([t0] * 5, [t0] * 5, [(1 << 32) - 1000] * 5)
    append(ctx, s, rs, rings[0])
    head, tail, btail = rs.head()[:2], rs.tail()[:2], rs.btail()[:2].astype(np.int64)
    if kind != "wrap32":
        head[1], btail[1] = {"ahead": (tail[1] + 5, btail[1]), "used>B": (0, btail[1] + B), "used<fill": (0, tail[1] - 1)}[kind]
        rs.set_counters(head, tail, btail & M32)
    x = drain_and_check(ctx, s, rs)
    assert (x["take"][2:5] > 0).all() and x["flags"] == (0 if kind == "wrap32" else lib.DR_BADCOUNT)
    assert (x["take"][1] > 600 and rs.head()[1] < D) if kind == "wrap32" else x["take"][1] == 0
    rs.free()


@pytest.mark.parametrize("what", ["pos16+1", "len"])
def test_bad_descriptor(rounds, what):
    """one queued frame of ring 1's second descriptor tile breaks the chain: USN_DR_BADDESC, nothing moves"""
    ctx, s, rings = rounds
    rs = ample(ctx)
    append(ctx, s, rs, rings[3])
    field = "pos16" if what == "pos16+1" else "lens"
    good = getattr(rs, field)()
    broken = good.copy()
    broken[512 + P + 188] += 1 if field == "pos16" else 16   # ring 1's descriptors start at 512
    upload(rs, field, broken)
    x = drain_and_check(ctx, s, rs)
    assert x["flags"] == lib.DR_BADDESC and x["take"][1] > 2 * P
    upload(rs, field, good)
    y = drain_and_check(ctx, s, rs)
    assert y["flags"] == 0 and np.array_equal(y["take"], x["take"])
    rs.free()


def test_tiny_and_absent_rings(rounds):
    """D = 1: a full ring taken whole ends at btail, not at the head's own descriptor"""
    ctx, s, rings = rounds
    rs = lib.DeviceBRingSet(ctx, [64, 1, 2, 8, 0], [256, 4, 8, 32, 0], poison=POISON)
    for _ in range(2):   # the second append lands because the first drain emptied the rings
        append(ctx, s, rs, rings[0])
        assert drain_and_check(ctx, s, rs)["take"][:5].tolist() == [0, 1, 2, 8, 0]
    rs.free()


def test_more_rings_than_one_lookup_block():
    """the byte-ring tests' 1100 more pipes with one-tile runs: both prefixes are looked up past id 1024"""
    ctx, s, _ = make_ctx()
    n = 40
    ring = add_ring(ctx, s, np.where(np.arange(n) % 8 == 0, ARP, EP + 1 + np.arange(n) % 4), stride=2048, lens=pool_lens(n, 6))
    for e in range(5, 1105):
        ctx.endpoint_add(e, lib.EP_PIPE, 0)
    rs = lib.DeviceBRingSet(ctx, [32] * 1105, [1024] * 1105, poison=POISON)
    append(ctx, s, rs, [ring])
    x = drain_and_check(ctx, s, rs, [M32] * 1105)
    assert (x["take"] > 0).sum() > 1024 and x["take"][1104] >= 5 and x["flags"] == 0
    ctx.close()
