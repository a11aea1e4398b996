#!/usr/bin/env python3
"""Device time of usn_deliver on classified calls of a config, next to a
device-to-device copy of the same n x slot bytes (the yardstick: the gather
moves the same frame bytes plus 6 B/frame of index and lens read and 6 B/frame
of src and lens written) and to the classify + lists call that precedes it.

A call is `--multi` rings of `--frames` frames classified by one
usn_classify_multi (c5: 2 x 8M, c2: 8 x 1M), then one usn_deliver per ring.
Inputs, results and deliveries rotate over `--rounds` distinct device sets
(> the 256 MiB Infinity Cache in all); deliver and copy alternate in blocks so
both see the same neighbours.  Times are device events on the one stream.

--packed times usn_deliver_packed (byte-compact rings) on the same calls next
to two yardsticks: usn_deliver of the same rings at --slot (2048 for c3) and a
device-to-device copy of need_bytes, the three alternating in blocks.

--round times usn_deliver_round (the call's rings as one poll round: one ring
per endpoint, two launches) next to the loop of --multi usn_deliver calls on
the same rings and results, and to ONE device-to-device copy of the same
need x slot bytes, the three alternating in blocks.

--rings times usn_deliver_rings (the round appended to persistent endpoint
rings: three launches) next to usn_deliver_round on the same rings and results
and to ONE device-to-device copy of the accepted bytes, alternating in blocks:
once with rings ample enough that nothing drops, once with rings of about half
of what each endpoint is offered.  Heads are reset to the tails between calls
(a device copy outside the timed span), so the rings never fill up.

--drain times usn_rings_drain (the consumer: four launches) with full budgets on
--rings' ample ring sets next to the usn_deliver_rings append that filled them
and to ONE device-to-device copy of need_bytes, the three alternating in blocks.
Every timed drain follows an append and every timed append a drain, each
outside the other's timed span: the drain moves the heads itself.

--brings times usn_deliver_brings (the round appended to persistent BYTE-COMPACT
rings: five launches) next to usn_deliver_rings at --slot on the same rings and
results and to ONE device-to-device copy of 16 x accepted_units bytes,
alternating in blocks: once with ample rings, once with byte rings of the power
of two nearest half of each endpoint's offered units.  Heads are reset as for
--rings.  The sets' sizes in bytes and the spread of the ring mode's own block
medians are recorded next to the times.

--bdrain times usn_brings_drain (the byte rings' consumer: three launches) with
full budgets on --brings' ample byte rings next to ONE device-to-device copy of
need_bytes and, where no frame is longer than --slot, to usn_rings_drain of the
same frames out of --drain's slot rings in the same run, alternating in blocks.
Every timed drain follows an untimed append of its own family.

usage: python tools/deliver_bench.py [--config c5] [--frames N] [--multi 2] [--rounds 2]
                                     [--launches 120] [--slot 64]
                                     [--packed | --round | --rings | --drain | --brings | --bdrain]
                                     [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from usnetd_amd import lib, traffic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c5")
    ap.add_argument("--frames", type=int, default=1 << 23)
    ap.add_argument("--multi", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--launches", type=int, default=120)
    ap.add_argument("--slot", type=int, default=64)
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--round", action="store_true")
    ap.add_argument("--rings", action="store_true")
    ap.add_argument("--drain", action="store_true")
    ap.add_argument("--brings", action="store_true")
    ap.add_argument("--bdrain", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    n, Q, R = a.frames, a.multi, a.rounds
    cfgs = [traffic.config(a.config, n=n, seed=17 * k + 2) for k in range(Q)]
    ctx = lib.Ctx(0)
    traffic.install_ctx(ctx, cfgs[0])
    nics = [cfgs[0].src] + list(traffic.extra_nics(cfgs[0], Q - 1, ctx))
    n_ep = max(nics) + 1
    s = ctx.stream()
    # R device sets of the call's rings, results and deliveries
    bs = [[lib.DeviceBatch(ctx, c.frames, c.lens, nics[k], stride=c.stride) for k, c in enumerate(cfgs)]
          for _ in range(R)]
    rs = [[lib.DeviceResult(ctx, n, max_endpoints=n_ep) for _ in range(Q)] for _ in range(R)]
    dvs = [[lib.DeviceDelivery(ctx, n, a.slot) for _ in range(Q)] for _ in range(R)]
    copy_src = [[b.buf.ptr for b in row] for row in bs]
    copy_dst = [[d.desc.frames for d in row] for row in dvs]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    if a.packed:
        # a frame is delivered at most once here (the tool's configs flood nothing): n slots and
        # the ring's sum of ceil16(len) bytes hold any delivery
        room = [int(((c.lens.astype(np.int64) + 15) // 16 * 16).sum()) for c in cfgs]
        pds = [[lib.DevicePackedDelivery(ctx, n, room[k]) for k in range(Q)] for _ in range(R)]
        need_b = [0] * Q   # per ring, after the first delivery

    def classify(r):
        ctx.classify_multi(bs[r], rs[r], s)

    def deliver(r):
        for k in range(Q):
            ctx.deliver(bs[r][k], rs[r][k], dvs[r][k], s)

    def copy(r):
        for k in range(Q):
            assert hip.hipMemcpyDtoDAsync(copy_dst[r][k], copy_src[r][k], n * a.slot, s) == 0

    def deliver_packed(r):
        for k in range(Q):
            ctx.deliver_packed(bs[r][k], rs[r][k], pds[r][k], s)

    def copy_packed(r):
        for k in range(Q):
            assert hip.hipMemcpyDtoDAsync(pds[r][k].desc.frames, copy_src[r][k], need_b[k], s) == 0

    def timed(fn, count, after=None, before=None):
        evs = [(ctx.event(), ctx.event()) for _ in range(count)]
        for i, (x, y) in enumerate(evs):
            if before:
                before(i % R)
            ctx.record(x, s)
            fn(i % R)
            ctx.record(y, s)
            if after:
                after(i % R)
        ctx.sync(s)
        return [ctx.elapsed_ms(x, y) * 1e3 for x, y in evs]

    def finalize(r):
        for k in range(Q):
            ctx.finalize(bs[r][k], rs[r][k], s)

    for r in list(range(R)) * 2:   # warm-up: every set classified, delivered and copied
        classify(r)
        finalize(r)
        deliver(r)
        copy(r)
    ctx.sync(s)
    cls_us = timed(classify, max(20, 2 * R), after=finalize)
    # what the deliveries hold: the header, and the slots against the lists
    need = 0
    for r in range(R):
        deliver(r)
        for k in range(Q):
            h = dvs[r][k].info(s)
            off = rs[r][k].bin_off()
            assert h.need == int(off[int(rs[r][k].summary()["n_ep"])]), "need differs from the endpoint bins"
            need += h.need if r == 0 else 0
    src0, len0, _ = dvs[0][0].ring(2)
    assert np.array_equal(src0, rs[0][0].lists().get(2, np.zeros(0, np.uint32)))
    assert np.array_equal(len0, cfgs[0].lens[src0])
    block = 30
    if a.packed:
        return packed(a, ctx, s, cfgs, rs, pds, need_b, need, deliver, deliver_packed, copy_packed,
                      timed, block)
    if a.round:
        return round_mode(a, ctx, s, hip, bs, rs, dvs, need, deliver, timed, block)
    if a.rings:
        return rings_mode(a, ctx, s, hip, bs, rs, need, timed, block)
    if a.drain:
        return drain_mode(a, ctx, s, hip, bs, rs, need, timed, block)
    if a.brings:
        return brings_mode(a, ctx, s, hip, bs, rs, need, timed, block)
    if a.bdrain:
        return bdrain_mode(a, ctx, s, hip, bs, rs, need, timed, block)
    dl_us, cp_us = [], []
    while len(dl_us) < a.launches:
        dl_us += timed(deliver, block)
        cp_us += timed(copy, block)
    frames = n * Q
    dl, cp, cl = (statistics.median(x) for x in (dl_us, cp_us, cls_us))
    moved = need * (2 * a.slot + 12)          # frame read + write, index + lens read, src + lens written
    out = dict(config=a.config, frames_per_call=frames, rings=Q, slot=a.slot, delivered_slots=need,
               deliver_us=round(dl, 1), deliver_min_us=round(min(dl_us), 1),
               deliver_p90_us=round(float(np.percentile(dl_us, 90)), 1), deliver_launches=len(dl_us),
               deliver_bytes_per_frame=round(moved / frames, 1), deliver_gbps=round(moved / dl / 1e3, 1),
               d2d_copy_us=round(cp, 1), d2d_copy_min_us=round(min(cp_us), 1),
               d2d_copy_gbps=round(2 * frames * a.slot / cp / 1e3, 1),
               deliver_over_copy=round(dl / cp, 2), classify_lists_us=round(cl, 1),
               deliver_share_of_call=round(dl / (dl + cl), 3))
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    ctx.close()


def stats(us, name):
    return {name + "_us": round(statistics.median(us), 1), name + "_min_us": round(min(us), 1),
            name + "_p90_us": round(float(np.percentile(us, 90)), 1)}


def round_mode(a, ctx, s, hip, bs, rs, dvs, need, deliver, timed, block):
    """usn_deliver_round against the loop of usn_deliver calls and one copy of need x slot bytes"""
    n, Q, R = a.frames, a.multi, a.rounds
    rds = [lib.DeviceRoundDelivery(ctx, n * Q, a.slot) for _ in range(R)]
    cp_src = ctx.alloc(need * a.slot)

    def deliver_round(r):
        ctx.deliver_round(bs[r], rs[r], rds[r], s)

    def copy_round(r):
        assert hip.hipMemcpyDtoDAsync(rds[r].desc.frames, cp_src.ptr, need * a.slot, s) == 0

    for r in list(range(R)) * 2:   # warm-up, and what the round holds against the per-ring deliveries
        deliver_round(r)
        copy_round(r)
    deliver(0)
    deliver_round(0)
    assert rds[0].info(s).need == need, "need differs from the sum of the rings' needs"
    for e in (2, int(rs[0][0].summary()["n_ep"]) - 1):
        src, lens, slots, ring = rds[0].ring(e)
        per = [dvs[0][k].ring(e) for k in range(Q)]
        assert np.array_equal(ring, np.repeat(np.arange(Q), [p[0].size for p in per]))
        for i, got in enumerate((src, lens, slots)):
            assert np.array_equal(got, np.concatenate([p[i] for p in per])), "round ring differs from its segments"
    rd_us, lp_us, cp_us = [], [], []
    while len(rd_us) < a.launches:
        rd_us += timed(deliver_round, block)
        lp_us += timed(deliver, block)
        cp_us += timed(copy_round, block)
    out = dict(config=a.config, frames_per_call=n * Q, rings=Q, slot=a.slot, delivered_slots=need,
               launches=len(rd_us), launches_per_call_round=2, launches_per_call_loop=2 * Q)
    out.update(stats(rd_us, "round"))
    out.update(stats(lp_us, "deliver_loop"))
    out.update(stats(cp_us, "d2d_copy"))
    out["round_over_loop"] = round(out["round_us"] / out["deliver_loop_us"], 3)
    out["round_over_copy"] = round(out["round_us"] / out["d2d_copy_us"], 2)
    out["loop_over_copy"] = round(out["deliver_loop_us"] / out["d2d_copy_us"], 2)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    ctx.close()


def rings_mode(a, ctx, s, hip, bs, rs, need, timed, block):
    """usn_deliver_rings (ample rings, then rings that drop about half) against usn_deliver_round
    and one copy of the accepted bytes"""
    n, Q, R = a.frames, a.multi, a.rounds
    rds = [lib.DeviceRoundDelivery(ctx, n * Q, a.slot) for _ in range(R)]
    ctx.deliver_round(bs[0], rs[0], rds[0], s)
    assert rds[0].info(s).need == need
    cnt = np.diff(rds[0].ep_off().astype(np.int64), append=need)   # what a call offers each endpoint
    ids = int(np.flatnonzero(cnt)[-1]) + 1
    pow2 = lambda v: np.where(v > 0, 2 ** np.ceil(np.log2(np.maximum(v, 1))), 0).astype(np.uint32)
    ample = pow2(cnt[:ids])
    half = pow2(np.where(cnt[:ids] > 0, np.maximum(cnt[:ids] / 2 ** 1.5, 1), 0))   # the power of two nearest cnt / 2
    sets = {"rings": [lib.DeviceRingSet(ctx, ample, a.slot) for _ in range(R)],
            "rings_half": [lib.DeviceRingSet(ctx, half, a.slot) for _ in range(R)]}
    cp_src = ctx.alloc(need * a.slot)
    hdrs = {}

    def deliver_round(r):
        ctx.deliver_round(bs[r], rs[r], rds[r], s)

    def copy(r, slots=need):
        assert hip.hipMemcpyDtoDAsync(rds[r].desc.frames, cp_src.ptr, slots * a.slot, s) == 0

    def rings(name):
        return lambda r: ctx.deliver_rings(bs[r], rs[r], sets[name][r], s)

    def drain(name):   # head = tail on the stream, outside the timed span
        def f(r):
            d = sets[name][r].desc
            assert hip.hipMemcpyDtoDAsync(d.head, d.tail, 4 * (lib.USN_MAX_ENDPOINTS + 1), s) == 0
        return f

    # the first append (heads 0) against the round delivery: two endpoints' rings
    for name in sets:
        rings(name)(0)
        hdrs[name] = sets[name][0].info(s, strict=False)
    assert (hdrs["rings"].accepted, hdrs["rings"].flags) == (need, 0), "the ample rings dropped or truncated"
    for e in (2, ids - 1):
        src, lens, slots, _ = rds[0].ring(e)
        for name, rsz in (("rings", ample), ("rings_half", half)):
            k = min(int(rsz[e]), lens.size)
            for got, want in zip(sets[name][0].ring(e), (lens, src, slots)):
                assert np.array_equal(got, want[:k]), "ring %d differs from the round delivery's" % e
    acc_half = int(hdrs["rings_half"].accepted)
    for name in sets:
        for r in list(range(R)) * 2:   # warm-up
            drain(name)(r)
            rings(name)(r)
        for r in range(R):
            drain(name)(r)
    us = {k: [] for k in ("rings", "round", "d2d_copy", "rings_half", "d2d_copy_half")}
    while len(us["rings"]) < a.launches:
        us["rings"] += timed(rings("rings"), block, after=drain("rings"))
        us["round"] += timed(deliver_round, block)
        us["d2d_copy"] += timed(copy, block)
        us["rings_half"] += timed(rings("rings_half"), block, after=drain("rings_half"))
        us["d2d_copy_half"] += timed(lambda r: copy(r, acc_half), block)
    for r in range(R):   # the last timed calls: nothing dropped from the ample rings, the same share from the others
        assert sets["rings"][r].info(s).accepted == need
        assert sets["rings_half"][r].info(s, strict=False).accepted == acc_half
    out = dict(config=a.config, frames_per_call=n * Q, rings=Q, slot=a.slot, offered_slots=need,
               endpoints_with_a_ring=int((ample > 0).sum()), ring_slots_ample=int(ample.sum()),
               ring_slots_half=int(half.sum()), accepted_half=acc_half,
               dropped_share_half=round(1 - acc_half / max(need, 1), 3), launches=len(us["rings"]),
               launches_per_call_rings=3, launches_per_call_round=2)
    for k, v in us.items():
        out.update(stats(v, k))
    out["rings_over_round"] = round(out["rings_us"] / out["round_us"], 3)
    out["rings_over_copy"] = round(out["rings_us"] / out["d2d_copy_us"], 2)
    out["rings_half_over_rings"] = round(out["rings_half_us"] / out["rings_us"], 3)
    out["rings_half_over_copy"] = round(out["rings_half_us"] / out["d2d_copy_half_us"], 2)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    ctx.close()


def drain_mode(a, ctx, s, hip, bs, rs, need, timed, block):
    """usn_rings_drain with full budgets on ample ring sets against the usn_deliver_rings append of
    the same frames and one copy of need_bytes"""
    n, Q, R = a.frames, a.multi, a.rounds
    rd = lib.DeviceRoundDelivery(ctx, n * Q, a.slot)
    ctx.deliver_round(bs[0], rs[0], rd, s)
    assert rd.info(s).need == need
    cnt = np.diff(rd.ep_off().astype(np.int64), append=need)   # what a call offers each endpoint
    rd.free()
    ids = int(np.flatnonzero(cnt)[-1]) + 1
    ample = np.where(cnt[:ids] > 0, 2 ** np.ceil(np.log2(np.maximum(cnt[:ids], 1))), 0).astype(np.uint32)
    sets = [lib.DeviceRingSet(ctx, ample, a.slot) for _ in range(R)]
    drs = [lib.DeviceDrain(ctx, need, need * a.slot) for _ in range(R)]
    for d in drs:
        d.set_budget([0xFFFFFFFF] * ids)
    cp_src = ctx.alloc(need * a.slot)

    def append(r):
        ctx.deliver_rings(bs[r], rs[r], sets[r], s)

    def drain(r):
        ctx.drain_rings(sets[r], drs[r], s)

    # the first append's rings against what the drain takes out of them: two endpoints
    append(0)
    assert (sets[0].info(s).accepted, sets[0].info(s).flags) == (need, 0), "the ample rings dropped or truncated"
    queued = {e: sets[0].ring(e) for e in (2, ids - 1)}
    drain(0)
    h = drs[0].info(s)
    assert (h.selected, h.taken, h.flags) == (need, need, 0) and not sets[0].ring(2)[0].size
    need_b = int(h.need_bytes)
    off, boff = drs[0].ep_off(), drs[0].ep_boff()
    for e, (lens, src, slots) in queued.items():
        k0, k1 = int(off[e]), int(off[e + 1])
        assert np.array_equal(drs[0].lens(k0, k1), lens) and np.array_equal(drs[0].src(k0, k1), src)
        want = np.concatenate([row[:(int(ln) + 15) // 16 * 16] for row, ln in zip(slots, lens)])
        assert np.array_equal(drs[0].bytes(int(boff[e]), int(boff[e + 1])), want), "ring %d drained differently" % e

    def copy(r):
        assert hip.hipMemcpyDtoDAsync(drs[r].desc.frames, cp_src.ptr, need_b, s) == 0

    for r in list(range(1, R)) + list(range(R)) * 2:   # warm-up; every set ends drained
        append(r)
        drain(r)
        copy(r)
    us = {k: [] for k in ("drain", "append", "d2d_copy")}
    while len(us["drain"]) < a.launches:
        us["drain"] += timed(drain, block, before=append)
        us["append"] += timed(append, block, after=drain)
        us["d2d_copy"] += timed(copy, block)
    for r in range(R):   # the last calls took everything
        h = drs[r].info(s)
        assert (h.taken, h.need_bytes, h.flags) == (need, need_b, 0) and sets[r].info(s).accepted == need
    out = dict(config=a.config, frames_per_call=n * Q, rings=Q, slot=a.slot, drained_slots=need,
               need_bytes=need_b, endpoints_with_a_ring=int((ample > 0).sum()), ring_slots=int(ample.sum()),
               launches=len(us["drain"]), launches_per_call_drain=4, launches_per_call_append=3)
    for k, v in us.items():
        out.update(stats(v, k))
    out["drain_over_copy"] = round(out["drain_us"] / out["d2d_copy_us"], 2)
    out["append_over_copy"] = round(out["append_us"] / out["d2d_copy_us"], 2)
    out["drain_over_append"] = round(out["drain_us"] / out["append_us"], 3)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    ctx.close()


def brings_mode(a, ctx, s, hip, bs, rs, need, timed, block):
    """usn_deliver_brings (ample rings, then byte rings of about half the offered units) against
    usn_deliver_rings at --slot and one copy of the accepted units"""
    n, Q, R = a.frames, a.multi, a.rounds
    rd = lib.DeviceRoundDelivery(ctx, n * Q, a.slot)
    ctx.deliver_round(bs[0], rs[0], rd, s)
    assert rd.info(s).need == need
    off = rd.ep_off().astype(np.int64)
    cnt = np.diff(off, append=need)                            # frames a call offers each endpoint
    u = np.maximum(1, (rd.lens(0, need).astype(np.int64) + 15) // 16)
    csum = np.concatenate([[0], np.cumsum(u)])
    units = csum[np.minimum(off + cnt, need)] - csum[np.minimum(off, need)]   # ... and units
    rd.free()
    ids = int(np.flatnonzero(cnt)[-1]) + 1
    cnt, units = cnt[:ids], units[:ids]
    pow2 = lambda v: np.where(v > 0, 2 ** np.ceil(np.log2(np.maximum(v, 1))), 0).astype(np.uint32)
    D, B = pow2(cnt), pow2(units)
    Bh = pow2(np.where(units > 0, np.maximum(units / 2 ** 1.5, 1), 0))   # the power of two nearest units / 2
    sets = {"brings": [lib.DeviceBRingSet(ctx, D, B) for _ in range(R)],
            "brings_half": [lib.DeviceBRingSet(ctx, D, Bh) for _ in range(R)],
            "rings": [lib.DeviceRingSet(ctx, D, a.slot) for _ in range(R)]}
    total_u = int(units.sum())
    cp_src, cp_dst = ctx.alloc(16 * total_u), ctx.alloc(16 * total_u)

    def call(name):
        f = ctx.deliver_rings if name == "rings" else ctx.deliver_brings
        return lambda r: f(bs[r], rs[r], sets[name][r], s)

    def drain(name):   # head = tail on the stream, outside the timed span
        def f(r):
            d = sets[name][r].desc
            assert hip.hipMemcpyDtoDAsync(d.head, d.tail, 4 * (lib.USN_MAX_ENDPOINTS + 1), s) == 0
        return f

    def copy(nu):
        return lambda r: hip.hipMemcpyDtoDAsync(cp_dst.ptr, cp_src.ptr, 16 * nu, s)

    # the first append (heads 0): the headers, and the smallest ring against the ring mode's
    hdrs = {}
    for name in sets:
        call(name)(0)
        hdrs[name] = sets[name][0].info(s, strict=False)
    hb = hdrs["brings"]
    assert (hb.accepted, hb.accepted_units, hb.flags) == (need, total_u, 0), "the ample byte rings dropped"
    assert (hdrs["rings"].accepted, hdrs["rings"].flags) == (need, 0), "the ample rings dropped or truncated"
    e = int(np.argmin(np.where(cnt > 0, cnt, cnt.max() + 1)))
    lens, src, slots = sets["rings"][0].ring(e)
    blens, bsrc, body = sets["brings"][0].ring(e)
    assert np.array_equal(blens, lens) and np.array_equal(bsrc, src), "ring %d differs from the ring mode's" % e
    assert all(np.array_equal(b, row[:b.size]) for b, row in zip(body, slots)), "ring %d: bytes differ" % e
    acc_half, units_half = int(hdrs["brings_half"].accepted), int(hdrs["brings_half"].accepted_units)
    for name in sets:
        for r in list(range(R)) * 2:   # warm-up
            drain(name)(r)
            call(name)(r)
        for r in range(R):
            drain(name)(r)
    us = {k: [] for k in ("brings", "rings", "d2d_copy", "brings_half", "d2d_copy_half")}
    while len(us["brings"]) < a.launches:
        us["brings"] += timed(call("brings"), block, after=drain("brings"))
        us["rings"] += timed(call("rings"), block, after=drain("rings"))
        us["d2d_copy"] += timed(copy(total_u), block)
        us["brings_half"] += timed(call("brings_half"), block, after=drain("brings_half"))
        us["d2d_copy_half"] += timed(copy(units_half), block)
    for r in range(R):   # the last timed calls: nothing dropped from the ample rings, the same share from the others
        assert sets["brings"][r].info(s).accepted_units == total_u
        assert sets["brings_half"][r].info(s, strict=False).accepted_units == units_half
    blocks = [statistics.median(us["rings"][i:i + block]) for i in range(0, len(us["rings"]), block)]
    out = dict(config=a.config, frames_per_call=n * Q, rings=Q, slot=a.slot, offered_frames=need,
               offered_units=total_u, bytes_per_offered_frame=round(16 * total_u / max(need, 1), 1),
               endpoints_with_a_ring=int((D > 0).sum()), descriptors=int(D.sum()), units_ample=int(B.sum()),
               units_half=int(Bh.sum()), accepted_half=acc_half, accepted_units_half=units_half,
               dropped_share_half=round(1 - acc_half / max(need, 1), 3),
               bringset_bytes=int(sets["brings"][0].nbytes), bringset_half_bytes=int(sets["brings_half"][0].nbytes),
               ringset_bytes=int(ctx.L.usn_ringset_bytes(max(int(D.sum()), 1), a.slot)),
               launches=len(us["brings"]), launches_per_call_brings=5, launches_per_call_rings=3,
               rings_block_medians_us=[round(b, 1) for b in blocks],
               rings_block_p10_us=round(float(np.percentile(blocks, 10)), 1),
               rings_block_p90_us=round(float(np.percentile(blocks, 90)), 1))
    out["footprint_ratio"] = round(out["ringset_bytes"] / out["bringset_bytes"], 2)
    for k, v in us.items():
        out.update(stats(v, k))
    out["brings_over_rings"] = round(out["brings_us"] / out["rings_us"], 3)
    out["brings_over_copy"] = round(out["brings_us"] / out["d2d_copy_us"], 2)
    out["brings_half_over_copy"] = round(out["brings_half_us"] / out["d2d_copy_half_us"], 2)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    ctx.close()


def bdrain_mode(a, ctx, s, hip, bs, rs, need, timed, block):
    """usn_brings_drain with full budgets on ample byte rings against one copy of need_bytes and, where
    the frames fit --slot, usn_rings_drain of the same frames out of slot rings"""
    n, Q, R = a.frames, a.multi, a.rounds
    rd = lib.DeviceRoundDelivery(ctx, n * Q, a.slot)
    ctx.deliver_round(bs[0], rs[0], rd, s)
    assert rd.info(s, strict=False).need == need
    off = rd.ep_off().astype(np.int64)
    cnt = np.diff(off, append=need)                            # frames a call offers each endpoint
    lens = rd.lens(0, need).astype(np.int64)
    u = np.maximum(1, (lens + 15) // 16)
    csum = np.concatenate([[0], np.cumsum(u)])
    units = csum[np.minimum(off + cnt, need)] - csum[np.minimum(off, need)]   # ... and units
    rd.free()
    ids = int(np.flatnonzero(cnt)[-1]) + 1
    pow2 = lambda v: np.where(v > 0, 2 ** np.ceil(np.log2(np.maximum(v, 1))), 0).astype(np.uint32)
    D, B, total_u = pow2(cnt[:ids]), pow2(units[:ids]), int(units.sum())
    with_slot = int(lens.max()) <= a.slot and int(lens.min()) > 0   # then both drains lay out the same bytes
    sets = [lib.DeviceBRingSet(ctx, D, B) for _ in range(R)]
    drs = [lib.DeviceDrain(ctx, need, 16 * total_u) for _ in range(R)]
    ssets = [lib.DeviceRingSet(ctx, D, a.slot) for _ in range(R)] if with_slot else []
    sdrs = [lib.DeviceDrain(ctx, need, need * a.slot) for _ in range(R)] if with_slot else []
    for d in drs + sdrs:
        d.set_budget([0xFFFFFFFF] * ids)
    cp_src = ctx.alloc(16 * total_u)

    def append(r):
        ctx.deliver_brings(bs[r], rs[r], sets[r], s)

    def bdrain(r):
        ctx.drain_brings(sets[r], drs[r], s)

    def sappend(r):
        ctx.deliver_rings(bs[r], rs[r], ssets[r], s)

    def sdrain(r):
        ctx.drain_rings(ssets[r], sdrs[r], s)

    def copy(r):
        assert hip.hipMemcpyDtoDAsync(drs[r].desc.frames, cp_src.ptr, 16 * total_u, s) == 0

    # the first append's rings against what the drain takes out of them: two endpoints
    append(0)
    hb = sets[0].info(s)
    assert (hb.accepted, hb.accepted_units, hb.flags) == (need, total_u, 0), "the ample byte rings dropped"
    queued = {e: sets[0].ring(e) for e in (2, ids - 1)}
    bdrain(0)
    h = drs[0].info(s, brings=True)
    assert (h.selected, h.taken, h.need_bytes, h.flags) == (need, need, 16 * total_u, 0) and not sets[0].ring(2)[0].size
    eo, boff = drs[0].ep_off(), drs[0].ep_boff()
    for e, (qlens, qsrc, body) in queued.items():
        k0, k1 = int(eo[e]), int(eo[e + 1])
        assert np.array_equal(drs[0].lens(k0, k1), qlens) and np.array_equal(drs[0].src(k0, k1), qsrc)
        assert np.array_equal(drs[0].bytes(int(boff[e]), int(boff[e + 1])), np.concatenate(body)), \
            "ring %d drained differently" % e
    paths = [("bdrain", bdrain, append), ("d2d_copy", copy, None)] + ([("slot_drain", sdrain, sappend)] if with_slot else [])
    for r in list(range(1, R)) + list(range(R)) * 2:   # warm-up; every set ends drained
        for _, fn, before in paths:
            if before:
                before(r)
            fn(r)
    us = {name: [] for name, _, _ in paths}
    while len(us["bdrain"]) < a.launches:
        for name, fn, before in paths:
            us[name] += timed(fn, block, before=before)
    for r in range(R):   # the last calls took everything
        h = drs[r].info(s, brings=True)
        assert (h.taken, h.need_bytes, h.flags) == (need, 16 * total_u, 0)
        if with_slot:
            hs = sdrs[r].info(s)
            assert (hs.taken, hs.need_bytes, hs.flags) == (need, 16 * total_u, 0)
    ref = "slot_drain" if with_slot else "d2d_copy"   # the comparison path's own spread in this run
    blocks = [statistics.median(us[ref][i:i + block]) for i in range(0, len(us[ref]), block)]
    out = dict(config=a.config, frames_per_call=n * Q, rings=Q, slot=a.slot, drained_frames=need,
               need_bytes=16 * total_u, endpoints_with_a_ring=int((D > 0).sum()), descriptors=int(D.sum()),
               units=int(B.sum()), unit_tile=lib.USN_BDRAIN_UTILE, launches=len(us["bdrain"]),
               launches_per_call_bdrain=3, launches_per_call_slot_drain=4, spread_of=ref,
               block_medians_us=[round(b, 1) for b in blocks])
    for k, v in us.items():
        out.update(stats(v, k))
    out["bdrain_over_copy"] = round(out["bdrain_us"] / out["d2d_copy_us"], 2)
    if with_slot:
        out["slot_drain_over_copy"] = round(out["slot_drain_us"] / out["d2d_copy_us"], 2)
        out["bdrain_over_slot_drain"] = round(out["bdrain_us"] / out["slot_drain_us"], 3)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    ctx.close()


def packed(a, ctx, s, cfgs, rs, pds, need_b, need, deliver, deliver_packed, copy_packed, timed, block):
    """usn_deliver_packed against usn_deliver at --slot and a copy of need_bytes"""
    n, Q, R = a.frames, a.multi, a.rounds
    for r in range(R):
        deliver_packed(r)
        for k in range(Q):
            h = pds[r][k].info(s)
            off = rs[r][k].bin_off()
            assert h.need == int(off[int(rs[r][k].summary()["n_ep"])]), "need differs from the endpoint bins"
            if r == 0:
                need_b[k] = int(h.need_bytes)
    # ring 0's bytes against the lists: every frame padded to 16 behind the one before
    lists, c = rs[0][0].lists(), cfgs[0]
    idx = np.concatenate([lists[e] for e in sorted(lists) if e < int(rs[0][0].summary()["n_ep"])])
    c16 = (c.lens[idx].astype(np.int64) + 15) // 16 * 16
    assert np.array_equal(pds[0][0].src(0, idx.size), idx) and int(c16.sum()) == need_b[0]
    assert np.array_equal(pds[0][0].off16(0, idx.size), (np.cumsum(c16) - c16) // 16)
    k = idx.size - 1
    f0 = int(idx[k]) * c.stride
    assert np.array_equal(pds[0][0].bytes(need_b[0] - int(c16[k]), need_b[0])[:c.lens[idx[k]]],
                          np.asarray(c.frames).reshape(-1)[f0:f0 + int(c.lens[idx[k]])])
    for r in range(R):   # warm-up of the copy at its final size
        copy_packed(r)
    pk_us, dl_us, cp_us = [], [], []
    while len(pk_us) < a.launches:
        pk_us += timed(deliver_packed, block)
        dl_us += timed(deliver, block)
        cp_us += timed(copy_packed, block)
    nb = sum(need_b)
    out = dict(config=a.config, frames_per_call=n * Q, rings=Q, slot=a.slot, delivered_slots=need,
               need_bytes=nb, need_x_slot_bytes=need * a.slot,
               bytes_per_delivered_frame=round(nb / max(need, 1), 1), launches=len(pk_us))
    out.update(stats(pk_us, "packed"))
    out.update(stats(dl_us, "fixed_slot"))
    out.update(stats(cp_us, "d2d_copy_need_bytes"))
    out["packed_over_fixed_slot"] = round(out["packed_us"] / out["fixed_slot_us"], 2)
    out["packed_over_copy"] = round(out["packed_us"] / out["d2d_copy_need_bytes_us"], 2)
    out["packed_frame_gbps"] = round(2 * nb / out["packed_us"] / 1e3, 1)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
