"""usn_rings_drain: the endpoint rings' queued frames gathered byte-compact, bit-exact
against plain numpy over the ring set AS FOUND: head, tail, lens, src and the slots are
read back before the call and the expectation follows from them alone, so nothing here
leans on the appends being right.  Every output is compared as a WHOLE array (the
selected entries, and that everything else keeps the poison), then from / take / left,
the header, head after the call, and that tail and the ring arrays did not change.
"""
import numpy as np
import pytest

from usnetd_amd import lib
import test_gpu_deliver as base
from test_gpu_deliver import ARP, DROP, EAPOL, EP, NIC, P, POISON
from test_gpu_deliver_round import add_ring, make_ctx

pytestmark = pytest.mark.gpu
IDS, M32, ALL = lib.USN_MAX_ENDPOINTS + 1, 0xFFFFFFFF, [0xFFFFFFFF] * 5


def ring_state(rs):
    return dict(head=rs.head().astype(np.int64), tail=rs.tail().astype(np.int64), lens=rs.lens(),
                src=rs.src(), slots=rs.slots())


def expect(rs, st, budget, cap):
    """the contract of usn_classify.h "ring drain" over the state st"""
    size = np.zeros(IDS, np.int64)
    size[:rs.off.size - 1] = np.diff(rs.off)
    bud = np.zeros(IDS, np.int64)
    bud[:len(budget)] = budget
    f = (st["tail"] - st["head"]) & M32
    avail = np.where(f <= size, f, 0)
    ep_off = np.minimum(np.concatenate([[0], np.cumsum(np.minimum(avail, bud))]), cap)
    take = np.diff(ep_off)
    q = np.concatenate([rs.off[e] + ((st["head"][e] + np.arange(take[e])) & (size[e] - 1))
                        for e in np.flatnonzero(take)] + [np.empty(0, np.int64)]).astype(np.int64)
    clen = np.minimum(st["lens"][q].astype(np.int64), rs.slot)
    boff = np.concatenate([[0], np.cumsum((clen + 15) // 16 * 16)])
    flags = (lib.DR_MORE if (avail > take).any() else 0) | (lib.DR_BADCOUNT if ((size > 0) & (f > size)).any() else 0) \
        | (lib.DV_LONG if (st["lens"][q] > rs.slot).any() else 0)
    return dict(take=take, left=avail - take, ep_off=ep_off, q=q, clen=clen, boff=boff, need=int(boff[-1]), flags=flags)


def drain_and_check(ctx, s, rs, budget=ALL, cap=None, cap_bytes=None):
    cap = rs.total if cap is None else cap
    cap_bytes = cap * rs.slot if cap_bytes is None else cap_bytes
    st = ring_state(rs)
    x = expect(rs, st, budget, cap)
    fits, sel = x["need"] <= cap_bytes, x["q"].size
    flags = x["flags"] | (0 if fits else lib.DV_OVERFLOW_BYTES)
    dr = lib.DeviceDrain(ctx, cap, cap_bytes, poison=POISON)
    dr.set_budget(budget, s)
    ctx.drain_rings(rs, dr, s)
    hdr = dr.info(s, strict=False)
    print("selected %d taken %d n_recv %d need_bytes %d / %d flags %d; id 1: from %d take %d left %d" % (
        hdr.selected, hdr.taken, hdr.n_recv, hdr.need_bytes, hdr.cap_bytes, hdr.flags, dr.from_()[1], dr.take()[1],
        dr.left()[1]))
    assert (hdr.need_bytes, hdr.cap_bytes, hdr.selected, hdr.taken) == (x["need"], cap_bytes, sel, sel if fits else 0)
    assert (hdr.n_recv, hdr.flags) == ((x["take"] > 0).sum(), flags)
    assert hdr.status == (lib.USN_ERANGE if flags & (lib.DV_OVERFLOW_BYTES | lib.DR_BADCOUNT) else 0)
    np.testing.assert_array_equal(dr.from_(), st["head"])
    np.testing.assert_array_equal(dr.take(), x["take"])
    np.testing.assert_array_equal(dr.left(), x["left"])
    np.testing.assert_array_equal(dr.ep_off(), x["ep_off"])
    np.testing.assert_array_equal(dr.ep_boff(), x["boff"][x["ep_off"]])
    for got, val, fill in ((dr.lens(), st["lens"][x["q"]], POISON * 0x0101), (dr.src(), st["src"][x["q"]], POISON * 0x01010101),
                           (dr.off16(), x["boff"][:-1] // 16, POISON * 0x01010101)):
        want = np.full(cap, fill, got.dtype)
        want[:sel] = val
        np.testing.assert_array_equal(got, want)
    want = np.full(cap_bytes, POISON, np.uint8)
    if fits:
        want[:x["need"]] = 0
        for o, n, k in zip(x["boff"], x["clen"], x["q"]):
            want[o:o + n] = st["slots"][k, :n]
    np.testing.assert_array_equal(dr.bytes(), want)
    after = ring_state(rs)
    np.testing.assert_array_equal(after.pop("head"), (st.pop("head") + (x["take"] if fits else 0)) & M32)
    for k in st:
        np.testing.assert_array_equal(after[k], st[k], k)
    dr.free()
    return x


def append(ctx, s, rs, rings):
    ctx.deliver_rings([g[0] for g in rings], [g[1] for g in rings], rs, s)
    return rs.info(s, strict=False)


@pytest.fixture(scope="module")
def rounds():
    """the rings tests' three-ring round (receiver 1 gets more than 2P frames, id 0 a few), and one ring"""
    ctx, s, _ = make_ctx()
    three = [add_ring(ctx, s, base.rx_kinds(1023)), add_ring(ctx, s, [ARP, EP + 1, EAPOL, NIC, EP + 3, ARP, DROP], src=2),
             add_ring(ctx, s, base.rx_kinds(2 * P + 5))]
    yield ctx, s, {1: [add_ring(ctx, s, base.rx_kinds(1025))], 3: three}
    ctx.close()


def mixed_rings(ctx, s):
    """test_layouts_and_long_frames' rings: lengths 14 .. 1514"""
    rng = np.random.default_rng(7)
    pool = np.array([14, 15, 16, 17, 31, 32, 33, 60, 64, 65, 127, 128])
    return [add_ring(ctx, s, base.rx_kinds(200)),
            add_ring(ctx, s, [EP + 1 + i % 4 if i % 3 else ARP for i in range(300)], stride=128,
                     lens=pool[rng.integers(0, pool.size, 300)], poison_in=True),
            add_ring(ctx, s, [EP + 1 + i % 4 if i % 5 else EAPOL for i in range(100)], offsets=True,
                     lens=np.array([60, 1024, 1025, 1514])[rng.integers(0, 4, 100)])]


@pytest.mark.parametrize("count", [1, 3])
def test_tiles(rounds, count):
    ctx, s, rings = rounds
    rs = lib.DeviceRingSet(ctx, [512, 2048, 512, 512, 512], 64, poison=POISON)
    assert append(ctx, s, rs, rings[count]).flags == 0
    x = drain_and_check(ctx, s, rs)
    assert x["flags"] == 0 and x["take"][1] > (2 * P if count > 1 else P) and (x["take"][2:5] > 0).all()
    assert drain_and_check(ctx, s, rs)["q"].size == 0   # everything is empty now: nothing is written
    rs.free()


@pytest.mark.parametrize("a", [700, 512, 1023, 1024 - 16])
def test_wrap(rounds, a):
    """ring 1 (1024 slots) takes a frames and is drained, takes about 700 more across its end and is
    drained again: the run wraps off any boundary, on a tile start, one slot before the end, 16 before it"""
    ctx, s, rings = rounds
    rs = lib.DeviceRingSet(ctx, [256, 1024, 256, 256, 256], 64, poison=POISON)
    append(ctx, s, rs, [add_ring(ctx, s, [EP + 1] * a)])
    assert drain_and_check(ctx, s, rs)["take"][1] == a
    assert append(ctx, s, rs, rings[1]).flags == 0   # lands only because the drain moved the head
    took = drain_and_check(ctx, s, rs)["take"][1]
    assert 600 < took and a + took > 1024
    rs.free()


@pytest.mark.parametrize("how", ["b0", "b1", "bP", "bP+37", "ball", "cap_in_1", "cap_at_1_end", "cap_in_0"])
def test_budget_and_cap(rounds, how):
    ctx, s, rings = rounds
    rs = lib.DeviceRingSet(ctx, [512, 2048, 512, 512, 512], 64, poison=POISON)
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


@pytest.mark.parametrize("slot", [1536, 128])
def test_mixed_lengths_and_long_frames(slot):
    ctx, s, _ = make_ctx()
    rs = lib.DeviceRingSet(ctx, [512] * 5, slot, poison=POISON)
    append(ctx, s, rs, mixed_rings(ctx, s))
    x = drain_and_check(ctx, s, rs)
    assert x["flags"] == (lib.DV_LONG if slot == 128 else 0) and np.unique(x["clen"]).size > (12 if slot > 128 else 8)
    ctx.close()


@pytest.mark.parametrize("delta", [-16, 0])
def test_byte_overflow(delta):
    ctx, s, _ = make_ctx()
    rs = lib.DeviceRingSet(ctx, [512] * 5, 1536, poison=POISON)
    append(ctx, s, rs, mixed_rings(ctx, s))
    need = expect(rs, ring_state(rs), ALL, rs.total)["need"]
    drain_and_check(ctx, s, rs, cap_bytes=need + delta)   # -16: nothing moves; 0: fits, poison from need_bytes on
    if delta:
        assert drain_and_check(ctx, s, rs, cap_bytes=need)["need"] == need   # still all there
    ctx.close()


@pytest.mark.parametrize("kind", ["wrap32", "ahead", "garbage"])
def test_counters(rounds, kind):
    """counters across the 2^32 wrap; a head ahead of the tail (USN_DR_BADCOUNT); rings nobody appended to,
    lens 0 .. 70 over poisoned slots (the pad is zero all the same) and poison lens that clamp to the slot"""
    ctx, s, rings = rounds
    rs = lib.DeviceRingSet(ctx, [256, 1024, 256, 256, 256], 64, poison=POISON)
    t0 = (1 << 32) - 300
    if kind == "wrap32":
        rs.set_counters([t0] * 5, [t0] * 5)
        append(ctx, s, rs, rings[1])
        x = drain_and_check(ctx, s, rs)
        assert x["take"][1] > 600 and rs.head()[1] < 1024
    elif kind == "ahead":
        rs.set_counters([0, t0 + 5, 0, 0, 0], [3, t0, 0, 200, 0])
        x = drain_and_check(ctx, s, rs)
        assert x["flags"] == lib.DR_BADCOUNT | lib.DV_LONG and x["take"][:4].tolist() == [3, 0, 0, 200]
    else:
        rs.buf.upload(np.arange(600, dtype=np.uint16) % 71, offset=rs.desc.lens - rs.buf.ptr + 2 * (256 + 500))
        rs.set_counters([t0, 900, 0, 0, 0], [t0 + 256, 900 + 1024, 0, 0, 256])
        x = drain_and_check(ctx, s, rs)
        assert x["flags"] == lib.DV_LONG and x["take"][:5].tolist() == [256, 1024, 0, 0, 256]
    rs.free()


def test_tiny_and_absent_rings(rounds):
    ctx, s, rings = rounds
    rs = lib.DeviceRingSet(ctx, [64, 1, 2, 8, 0], 64, poison=POISON)
    for _ in range(2):   # the second append lands because the first drain emptied the rings
        append(ctx, s, rs, rings[1])
        assert drain_and_check(ctx, s, rs)["take"][:5].tolist() == [0, 1, 2, 8, 0]
    rs.free()
