"""usn_deliver_packed: the rings of test_gpu_deliver.py, byte-compact.  One
checker restates the contract in numpy from the decisions the same result
holds and from lens: receivers and order as usn_deliver, off16 = exclusive sum
of ceil16(len) / 16, ep_boff, need_bytes, and frames[0, need_bytes) as the
frames zero-padded to 16 bytes behind one another.  Everything is exact, and
whatever lies past need / need_bytes keeps the poison.
"""
import numpy as np
import pytest

from usnetd_amd import lib
import test_gpu_deliver as base

pytestmark = pytest.mark.gpu
P = lib.USN_DELIVER_TILE
POISON = base.POISON
POOL = np.array([14, 15, 16, 17, 60, 64, 65, 576, 1500, 1514])
SIZES = [1, 1025, 3 * P + 1]


def pool_lens(n, seed=5):
    return POOL[np.random.default_rng(seed).integers(0, POOL.size, n)]


def deliver_and_check(st, regs, src, nic=0, cap_delta=3, bytes_delta=48):
    """deliver into need + cap_delta slots and need_bytes + bytes_delta bytes"""
    ctx, s, b, r, dec, F, lens, starts = st
    want = base.expected(dec, regs, src, nic)
    counts = np.zeros(lib.USN_MAX_ENDPOINTS, np.int64)
    for e, w in want.items():
        counts[e] = w.size
    idx = np.concatenate([want[e] for e in sorted(want)] + [np.zeros(0, np.int64)])
    need = idx.size
    off = np.concatenate([[0], np.cumsum((lens[idx].astype(np.int64) + 15) // 16 * 16)])
    need_bytes = int(off[-1])
    ep_off = np.concatenate([[0], np.cumsum(counts)])
    cap, cap_bytes = need + cap_delta, need_bytes + bytes_delta
    dv = lib.DevicePackedDelivery(ctx, cap, cap_bytes, poison=POISON)
    ctx.deliver_packed(b, r, dv, s)
    hdr = dv.info(s, strict=False)
    flags = lib.DV_OVERFLOW if need > cap else lib.DV_OVERFLOW_BYTES if need_bytes > cap_bytes else 0
    print("need %d slots, %d bytes, flags %d" % (hdr.need, hdr.need_bytes, hdr.flags))
    assert (hdr.need, hdr.n_recv, hdr.cap, hdr.cap_bytes) == (need, int((counts > 0).sum()), cap, cap_bytes)
    assert hdr.flags == flags and hdr.status == (lib.USN_ERANGE if flags else 0)
    assert hdr.need_bytes == (0 if flags == lib.DV_OVERFLOW else need_bytes)
    np.testing.assert_array_equal(dv.ep_off(), ep_off)
    k = 0 if flags == lib.DV_OVERFLOW else need          # slots whose src / lens / off16 are valid
    np.testing.assert_array_equal(dv.src()[:k], idx[:k])
    np.testing.assert_array_equal(dv.lens()[:k], lens[idx][:k])
    np.testing.assert_array_equal(dv.off16()[:k], (off[:-1] // 16)[:k])
    assert (dv.src()[k:] == POISON * 0x01010101).all() and (dv.lens()[k:] == POISON * 0x0101).all()
    assert (dv.off16()[k:] == POISON * 0x01010101).all()
    if k:
        np.testing.assert_array_equal(dv.ep_boff(), off[ep_off])
    else:
        assert (dv.ep_boff() == POISON * 0x0101010101010101).all()
    exp = np.zeros(need_bytes, np.uint8)
    for o, i in zip(off, idx):
        exp[o:o + lens[i]] = F[starts[i]:starts[i] + lens[i]]
    nb = 0 if flags else need_bytes
    got = dv.bytes()
    np.testing.assert_array_equal(got[:nb], exp[:nb])
    assert (got[nb:] == POISON).all()
    dv.free()
    return want


@pytest.mark.parametrize("offsets", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_rx_mixed_lengths_across_tile_cuts(n, offsets):
    """strided at 2048 with the input slot past len poisoned, and the offsets[] layout"""
    st = base.setup(base.rx_kinds(n), stride=2048, lens=pool_lens(n), offsets=offsets, poison_in=not offsets)
    want = deliver_and_check(st, range(5), 0)
    assert want[0].size == 0 and (n < 3 * P or want[1].size > 2 * P)
    st[0].close()


@pytest.mark.parametrize("length", [64, 60])
@pytest.mark.parametrize("n", SIZES)
def test_uniform_fast_path(n, length):
    """every tile has one piece count: 64 exactly, and 60 with its masked tail"""
    st = base.setup(base.rx_kinds(n), stride=64, lens=np.full(n, length), poison_in=True)
    deliver_and_check(st, range(5), 0)
    st[0].close()


def test_tx_three_way_merge():
    n = 2 * P + 3
    cyc = [base.EP + 3, base.NIC, base.ARP, base.EP + 0, base.NIC, base.EAPOL, base.DROP]
    lens = np.maximum(pool_lens(n), np.where(np.arange(n) % 7 == 2, 14, 60))   # short frames only where ARP
    st = base.setup([cyc[i % 7] for i in range(n)], src=2, stride=2048, lens=lens, nic_is_pipe=True)
    want = deliver_and_check(st, [0, 1, 2, 3, 4, 6], 2)
    assert set(((st[4][want[0]] >> 16) & 0xF).tolist()) == {lib.CLS_EP, lib.CLS_NIC, lib.CLS_FLOOD}
    assert want[0].size > P and want[2].size == 0
    st[0].close()


def test_more_tiles_than_one_scan_block():
    """1100 more pipes, each with a one-tile ring of the flooded frames: 1104 tiles"""
    n = 40
    kinds = np.where(np.arange(n) % 8 == 0, base.ARP, base.EP + 1 + np.arange(n) % 4)
    st = base.setup(kinds, stride=2048, lens=pool_lens(n, 6))
    for e in range(5, 1105):
        st[0].endpoint_add(e, lib.EP_PIPE, 0)
    want = deliver_and_check(st, range(1105), 0)
    assert sum(w.size > 0 for w in want.values()) > 1024 and want[1104].size >= 5
    st[0].close()


@pytest.mark.parametrize("cap_delta,bytes_delta", [(0, -16), (-1, 48), (0, 0)])
def test_overflow(cap_delta, bytes_delta):
    st = base.setup(base.rx_kinds(1025), stride=2048, lens=pool_lens(1025))
    deliver_and_check(st, range(5), 0, cap_delta=cap_delta, bytes_delta=bytes_delta)
    st[0].close()


def test_receiver_set_follows_the_context():
    st = base.setup(base.rx_kinds(1025), stride=2048, lens=pool_lens(1025))
    ctx, dec = st[0], st[4]
    deliver_and_check(st, range(5), 0)
    ctx.endpoint_remove(3)
    ctx.endpoint_add(5, lib.EP_PIPE, 0)
    want = deliver_and_check(st, [0, 1, 2, 4, 5], 0)
    assert ((dec & 0xFFFF) == 3).any()   # endpoint 3's bin is not empty; its ring is
    np.testing.assert_array_equal(want[5], np.flatnonzero((dec >> 16) & 0xF == lib.CLS_FLOOD))
    ctx.close()
