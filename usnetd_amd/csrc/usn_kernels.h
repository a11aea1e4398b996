/*
 * usn_kernels.h -- launch interface between the C++ host (usn_host.cpp) and
 * the HIP kernels (usn_device.hip).  Internal; not part of the C ABI.
 */
#ifndef USN_KERNELS_H
#define USN_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/usn_classify.h"
#include "usn_internal.h"

namespace usn {

enum CarryMode : uint32_t { CARRY_NONE = 0, CARRY_EXPLICIT = 1, CARRY_CHAIN = 2 };

struct ClassifyArgs {
  /* batch */
  const uint8_t *frames;
  uint64_t stride;
  const uint64_t *offsets;
  const uint16_t *lens;
  uint64_t n;
  uint32_t ntiles;
  uint32_t window;          /* readable bytes at every frame start (usn_batch.window) */
  uint32_t epoch;           /* the launch tag (ScatterArgs::epoch): a tile that lists frames for
                               the host stage stores it in summary->host_epoch */
  /* outputs */
  uint32_t *decisions;
  uint16_t *cnt;            /* [ntiles][nbw] frames per bin of each tile (the scatter's input) */
  uint32_t nbw;             /* row length of cnt: nbins rounded up to 8 */
  usn_tile_hdr *tiles;
  usn_summary *summary;
  uint32_t *host_list;      /* per tile USN_TILE slots */
  /* rule image (usn_internal.h): K1 / K2 perfect-hash tables in one buffer */
  const uint4 *table;
  uint32_t table_units;     /* 16-byte units of the K1/K2 image (U and X follow it) */
  uint32_t disp_unit;       /* first unit of the K1/K2 displacement arrays (up to table_units) */
  usn_ph_table ph[4];       /* K1 (key1 shapes), K2 (key2 shapes), U (projections), X (U overflow) */
  uint32_t u_disp_unit;     /* first unit of U's then X's displacements (probe_mask bit 2) */
  uint32_t u_end_unit;      /* end of the image */
  /* inner L2 bridge (tx): MACs in the low 48 bits */
  const uint64_t *bridge;
  uint32_t n_bridge;
  /* source endpoint */
  uint32_t src;
  uint32_t src_is_nic;
  uint32_t for_nic;
  uint32_t nbins;           /* endpoints + 3 */
  uint32_t nbits;           /* bits to tell bins apart (ceil log2 nbins) */
  uint32_t n_ep;            /* endpoints (bin of NIC) */
  uint32_t probe_mask;      /* bit0: K1 holds rules; bit1: K2 holds rules; bit2: U and X built */
  uint32_t next_dhcp_set;   /* the source's next_dhcp_endpoint is Some: DHCP answers need the host */
  /* carried 1-entry decision cache */
  uint32_t carry_mode;
  uint32_t cin_state, cin_dst;
  uint32_t cin_info[4];
  const usn_tile_hdr *prev_tiles;
  uint32_t prev_ntiles;
  const usn_summary *prev_summary;
};

/* Several batches (distinct sources) classified by one launch: workgroup w
 * takes tile w - tile_base[i] of batch i, tile_base[i] <= w < tile_base[i+1]. */
#define USN_MAX_MULTI 8
struct MultiArgs {
  ClassifyArgs b[USN_MAX_MULTI];
  uint32_t tile_base[USN_MAX_MULTI + 1];
  uint32_t count;
};
static_assert(sizeof(MultiArgs) <= 4096, "kernel argument block");

/* ---- tx direction (a non-NIC source sends): four launches ---------------- */
/* per-frame record, two planes of n uint4 written by tx_scan:
 *   rec[i]     r0 = {i0 | TXR_* flags, src, dst, ports}
 *   rec[n + i] r1 = {smac[0..3], smac[4..5] | dmac[0..1] << 16, dmac[2..5], 0}
 * r0 is all a frame's decision needs unless this batch learns a MAC (the
 * dmac test) or the frame is the first to learn one (its smac); in steady
 * state tx_hits and tx_decide read 16 B per frame, not 32.                   */
#define TXR_TOUCH_SHIFT 20u    /* 2 bits: 0 none, 1 retains, 2 leaves None, 3 unknown */
#define TXR_LEARNMAC (1u << 22)  /* unicast smac not in the bridge snapshot */
#define TXR_LEARNRULE (1u << 23) /* answer key not listened, not in the table snapshot */
#define TXR_HOST (1u << 24)      /* ordered host stage decides this frame */
#define TXR_SMAC_IN (1u << 25)
#define TXR_DMAC_IN (1u << 26)
#define TXR_HIT (1u << 27)       /* 1-entry cache hit (set by tx_hits) */
#define TXR_DHCPANS (1u << 28)
#define TXR_FRAG1 (1u << 29)     /* first fragment: extract_pkt_info remembers it (host map) */
#define TXR_WINDOW (1u << 30)    /* L4 ports lie past the batch window: the host reads the frame */
#define TXR_I0_MASK 0x1FFFFu

/* A tx launch takes one ring of the source, or up to USN_TX_RINGS consecutive
 * rings (rings > 1): workgroups [tile_base[k], tile_base[k + 1]) take ring k's
 * tiles.  The cross-tile protocol (aux granules, the learning sets' first
 * learners, learned items) runs over the launch's frame index: ring k's frame
 * j is tile_base[k] * USN_TILE + j; decisions, host lists, count rows and tile
 * headers are each ring's own. */
#define USN_TX_RINGS 8u
#define USN_TXC_HOST 4u         /* counters: frames ring k listed for the host stage, [4 + k] */
#define USN_TXC_LEARNED (USN_TXC_HOST + USN_TX_RINGS)   /* ... ring k's learned items (k >= 1) */
#define USN_TXC_WORDS (USN_TXC_LEARNED + USN_TX_RINGS)
struct TxArgs {
  ClassifyArgs a[USN_TX_RINGS];  /* ring k's batch and outputs; ring 0's also the shared
                                    fields: table, source, carried cache */
  uint32_t tile_base[USN_TX_RINGS + 1];
  uint32_t rings;
  unsigned long long *aux;    /* per tile x TXA_GRANULES {epoch, value}: what crosses a tile boundary */
  uint32_t *early;            /* per tile: epoch << 16 | EARLY, packed (the EARLY look-back reads
                                 four tiles per 16-byte load; granules would take one line each) */
  unsigned long long *macset; /* slots x 2: {epoch<<48 | mac, epoch<<32 | ~first} */
  unsigned long long *ruleset;/* slots x 4: {epoch<<48 | fp48, epoch<<32 | ~first, key xy, key zw} */
  uint32_t macset_mask, ruleset_mask;
  uint32_t epoch;             /* 1..65535 */
  uint4 *learned;             /* items appended by tx_decide: {frame, kind 0 mac | 1 rule},
                                 {mac lo, mac hi} or the packed rule key {x, y, z, meta} */
  uint32_t *counters;         /* USN_TXC_WORDS: [0] learned items, [1] overflow/collision flags,
                                 [2] sets with items, [3] epoch of a batch whose tile waits timed
                                 out, [USN_TXC_HOST + k] frames of ring k listed for the host
                                 stage, [USN_TXC_LEARNED + k] learned items of ring k >= 1's
                                 frames (ring 0's: [0] minus the others) */
  uint32_t learned_cap;
  const unsigned long long *bridge_set; /* open addressing, bit 63 = used */
  uint32_t bridge_mask;
  const uint32_t *listen;     /* n_listen x {dst, proto | has_port << 8 | port << 16} */
  uint32_t n_listen;
  uint32_t next_dhcp_set;     /* the source's next_dhcp_endpoint is Some */
};

#define TXA_GRANULES 24u       /* aux granules (8 bytes) per tile */
constexpr size_t TXA_WORDS_BYTES = TXA_GRANULES * 8;
constexpr size_t TXA_TILE_BYTES = TXA_WORDS_BYTES + 4;   /* + the tile's packed EARLY word */
static_assert(sizeof(TxArgs) <= 4096, "kernel argument block");
static_assert(USN_TXC_WORDS <= 64, "tile 0's first wave zeroes the counters");
hipError_t launch_tx(const TxArgs &t, hipStream_t stream);

/* LDS bytes a classify block needs (table staged in LDS when table_in_lds). */
size_t classify_lds_bytes(uint32_t nbins, uint32_t table_units, bool table_in_lds, bool glds);
bool table_fits_lds(uint32_t nbins, uint32_t table_units);

hipError_t launch_classify(const MultiArgs &m, hipStream_t stream);
/* Recount the bin rows and class counts of tiles [t0, t1) from the (patched)
 * decisions (the scatter then runs again). */
hipError_t launch_recount(const ClassifyArgs &a, uint32_t t0, uint32_t t1, hipStream_t stream);
/* table[idx[k]] = val[k] for the n units of buf = {val[n] (uint4)} {idx[n] (u32)} */
hipError_t launch_patch(uint4 *table, const void *buf, uint32_t n, hipStream_t stream);

/* ---- per-endpoint lists: the device-wide stable scatter ------------------
 * After the classify (or tx) kernel has written each tile's decisions and its
 * row of per-bin frame counts (cnt[tile][bin], u16), two launches:
 *   scan     (range of 16 x cpt chunks, block of USN_SCAN_BLK bins):
 *            agg[chunk][bin] = frames of the bin in the batch's chunks before
 *            (ranges hand their totals on through epoch-tagged granules),
 *            tot[bin] = the bin's frames
 *   scatter  (chunk of tc tiles): one LDS atomic per frame ranks it in the
 *            chunk's bin-sorted LDS stage (verified; ballot ranks as the
 *            fallback); the stage is written out in order, so each bin's
 *            frames of the chunk leave as one contiguous run
 * Stable: bins in order, frames in frame order inside a bin. */
#define USN_SCAN_RANGE_MIN 16u   /* chunks per scan workgroup: 16 x cpt (1, 2, 4) */
#define USN_SCAN_BLK 64u     /* bins per scan workgroup */
struct ScatterBatch {
  const uint32_t *decisions;
  const uint16_t *cnt;      /* [ntiles][nbw] */
  uint32_t *agg;            /* [nchunks][nbw]: frames per bin in the chunks before */
  uint32_t *tot;            /* [nbw]: frames per bin */
  unsigned long long *gran; /* [nranges][nbw]: {epoch, range total} */
  uint32_t *diag;           /* USN_DIAG_*: the lists are wrong (usn_finalize reports it) */
  uint32_t *index;          /* [n] */
  uint32_t *bin_off;        /* [nbins + 1] */
  uint32_t n, ntiles, tc, nchunks, nranges;
  /* an rx batch's state for usn_finalize, in host-mapped memory (or null):
   * [0] the launch tag, [1] summary flags, [2] USN_DIAG_LISTS when a chunk
   * found inconsistent lists, [3] 1 when a tile listed frames for the host
   * stage, [4..6] bin_off at the NIC, FLOOD and DROP bins, [7] the scan's
   * diag word.  Written by the scatter (chunk 0; [2] by any chunk). */
  uint32_t *rx_state;
  const usn_summary *summary;
};
struct ScatterArgs {
  ScatterBatch b[USN_MAX_MULTI];
  uint32_t chunk_base[USN_MAX_MULTI + 1];   /* scatter grid: chunks of batch i */
  uint32_t range_base[USN_MAX_MULTI + 1];   /* scan grid (x nbb): ranges of batch i */
  uint32_t count;
  uint32_t nbins, nbw, nbb, n_ep, nbits;
  uint32_t tc;                              /* the scatter kernel's chunk length for this launch */
  uint32_t flags;                           /* USN_SCF_* */
  uint32_t epoch;                           /* this launch's granule tag (never 0) */
  uint32_t cpt;                             /* scan: chunks per thread (1, 2, 4) */
  /* tx: chunk 0 of each batch (ring) also writes its state into host-mapped
   * memory for usn_finalize, USN_TXS_WORDS per ring: [0] summary flags,
   * [1] the ring's learned items, [2] counters[1] (flags), [3] counters[2],
   * [4] counters[3] (timeout epoch), [5] the ring's host-stage frames,
   * [6..8] bin_off[n_ep .. n_ep + 2], [9] n, [10] the scan's diag; word 11 of
   * ring 0's set by any chunk that finds inconsistent lists */
  uint32_t *txs_out;
  const uint32_t *txs_counters;
};
#define USN_TXS_WORDS 16u
#define USN_DIAG_TIMEOUT 1u     /* a scan wait timed out (200 ms; never observed) */
#define USN_DIAG_LISTS 2u       /* the scatter found count rows that disagree with the decisions */
#define USN_SCF_NOSCAN 2u      /* every batch is one chunk: no scan launch; the chunk's own counts
                                  are the batch's (agg = 0, tot = the chunk's sums) */
#define USN_SCF_SELFSCAN 4u    /* a small launch (every chunk resident at once, few count-row
                                  bytes per batch): no scan launch; each chunk sums its batch's
                                  count rows itself (the totals, and the tiles before it) */
#define USN_SCF_SLOW_RANK 1u   /* test hook (USN_SCATTER_SLOW_RANK=1): every chunk also ranks the
                                  ballot way and writes its stage out again */
/* The scatter kernel's chunk length (tc tiles, one wave each) for nbins
 * bins: the longest chunk (contiguous runs per bin) whose LDS -- stage
 * tc x 4 KiB | offsets nbw x 4 | cursors tc x nbw x 2 (| self-scan sums
 * nbw x 8) -- fits 64 KiB. */
struct ScatterShape { uint32_t tc; size_t lds; };
inline size_t scatter_lds(uint32_t nbins, uint32_t tc, bool selfscan = false) {
  const size_t nbw = (nbins + 7u) & ~7u;
  return (size_t)tc * USN_TILE * 4 + nbw * 4 + (size_t)tc * nbw * 2 + (selfscan ? nbw * 8 : 0);
}
inline ScatterShape scatter_shape(uint32_t nbins) {
  for (uint32_t tc : {8u, 4u, 2u})
    if (scatter_lds(nbins, tc) <= 64u * 1024u) return ScatterShape{tc, scatter_lds(nbins, tc)};
  return ScatterShape{1, scatter_lds(nbins, 1)};
}
inline uint32_t scatter_occupancy(size_t lds) {
  const uint32_t occ = (uint32_t)((160u * 1024u) / (lds ? lds : 1));
  return occ > 4 ? 4 : occ;
}
/* how a launch's lists are built (usn_host.cpp scatter_plan) */
struct ScatterPlan { uint32_t tc, cpt; bool noscan, selfscan; };
ScatterPlan scatter_plan(const uint32_t *ntiles, uint32_t count, uint32_t nbins, uint32_t cus,
                         uint32_t tc_knob, uint32_t cpt_knob, uint32_t selfscan_kb);
/* scratch bytes of one batch (cnt | agg | tot | gran | diag; agg and gran
 * sized for one-tile chunks) and its carve for chunks of tc tiles */
size_t scatter_scratch_bytes(uint64_t n, uint32_t nbins);
void scatter_carve(void *scratch, uint64_t cap, uint64_t n, uint32_t nbins, uint32_t tc, uint32_t cpt,
                   ScatterBatch &sb, uint16_t **cnt);
void scatter_tail(void *scratch, uint64_t cap, uint32_t nbins, void **p, size_t *bytes);
uint32_t *scatter_diag(void *scratch, uint64_t cap, uint32_t nbins);

/* ---- delivery (usn_deliver.hip): the per-endpoint output rings ------------
 * Two launches on the caller's stream:
 *   deliver_plan_kernel  one workgroup: per endpoint id the slots it receives
 *                        (its own bin, the NIC bin for the source's NIC, the
 *                        FLOOD bin for every registered id but the source),
 *                        their exclusive scan (ep_off), the header, and the
 *                        prefix of output tiles per receiver (tile_pfx)
 *   deliver_pack_kernel  a grid sized to the device; each workgroup loops
 *                        over output tiles of USN_DELIVER_TILE slots: finds
 *                        the tile's receiver and its cut into the receiver's
 *                        up to three sorted lists, merges the runs after the
 *                        cuts in LDS, writes src[] / lens[] and gathers the
 *                        frames with 128-bit loads and stores */
#define USN_DT_NONE 0xFFFFu     /* eptab[e]: id e is not registered */
#define USN_DT_NONIC 0xFFFEu    /* ... registered, a NIC itself (no for_nic) */
#define USN_DT_IDS (USN_MAX_ENDPOINTS + 1u)   /* 4096: ids scanned (the last is never registered) */
struct DeliverArgs {
  const uint8_t *frames;
  uint64_t stride;
  const uint64_t *offsets;
  const uint16_t *lens;
  uint32_t n;               /* frames in the batch (< 2^32 - 1) */
  uint32_t src;             /* the batch's source endpoint */
  const uint32_t *index;
  const uint32_t *bin_off;
  const usn_summary *summary;
  const uint16_t *eptab;    /* [USN_DT_IDS]: for_nic of a registered id, USN_DT_NONIC, USN_DT_NONE */
  uint8_t *out_frames;
  uint16_t *out_lens;
  uint32_t *out_src;
  uint32_t *ep_off;         /* [USN_DT_IDS] */
  usn_delivery_hdr *hdr;
  uint32_t *tile_pfx;       /* [USN_DT_IDS]: output tiles of the ids below; the last entry is
                               the tile total (0 on overflow) */
  uint32_t cap, slot;
};
/* bytes from usn_delivery.hdr to the plan's scratch (tile_pfx) */
constexpr size_t DELIVER_SCRATCH_OFF = 256;
constexpr size_t DELIVER_SCRATCH_BYTES = (size_t)USN_DT_IDS * 4;
hipError_t launch_deliver(const DeliverArgs &a, uint32_t pack_grid, hipStream_t stream);

/* ---- packed delivery (usn_deliver_packed.hip): byte-compact rings ----------
 * Four launches on the caller's stream, same receivers, order and tiles:
 *   pdeliver_plan_kernel   the plan above, plus need_bytes = 0 and cap_bytes
 *   pdeliver_merge_kernel  device-sized grid: per tile the cut and the merge,
 *                          src[] / lens[], and the tile's 16-byte pieces
 *                          (sum of ceil16(len) / 16) into tile_b16[t]
 *   pdeliver_scan_kernel   one workgroup: exclusive 64-bit scan of tile_b16 in
 *                          blocks of PDELIVER_SCAN_BLOCK tiles (tile_base),
 *                          ep_boff, need_bytes, the byte-overflow flag
 *   pdeliver_copy_kernel   device-sized grid: per tile src[] / lens[] read
 *                          back, the pieces' scan in LDS, off16[], and the
 *                          output-stationary gather (lane i of the tile's
 *                          pieces i, i + 256, ...) */
struct PackedDeliverArgs {
  const uint8_t *frames;
  uint64_t stride;
  const uint64_t *offsets;
  const uint16_t *lens;
  uint32_t n;               /* frames in the batch (< 2^32 - 1) */
  uint32_t src;             /* the batch's source endpoint */
  const uint32_t *index;
  const uint32_t *bin_off;
  const usn_summary *summary;
  const uint16_t *eptab;    /* as DeliverArgs */
  uint8_t *out_frames;
  uint32_t *out_off16;
  uint16_t *out_lens;
  uint32_t *out_src;
  uint32_t *ep_off;         /* [USN_DT_IDS] */
  uint64_t *ep_boff;        /* [USN_DT_IDS] */
  usn_pdelivery_hdr *hdr;
  uint32_t *tile_pfx;       /* [USN_DT_IDS], as DeliverArgs */
  uint64_t *tile_base;      /* [max tiles]: 16-byte pieces before tile t */
  uint32_t *tile_b16;       /* [max tiles]: 16-byte pieces of tile t (<= P * 4096) */
  uint32_t cap;
  uint64_t cap_bytes;
};
constexpr uint32_t PDELIVER_SCAN_BLOCK = 1024;   /* tiles per pass of the tile scan */
/* the most tiles a delivery of cap slots has: a receiver's last tile may be short */
constexpr size_t pdeliver_max_tiles(uint64_t cap) { return (size_t)(cap / USN_DELIVER_TILE) + USN_DT_IDS; }
/* scratch behind usn_pdelivery.hdr, from DELIVER_SCRATCH_OFF: tile_pfx, tile_base, tile_b16 */
constexpr size_t PDELIVER_BASE_OFF = DELIVER_SCRATCH_OFF + DELIVER_SCRATCH_BYTES;   /* 8-byte aligned */
constexpr size_t pdeliver_scratch_bytes(uint64_t cap) {
  return DELIVER_SCRATCH_BYTES + pdeliver_max_tiles(cap) * 12;
}
hipError_t launch_deliver_packed(const PackedDeliverArgs &a, uint32_t grid, hipStream_t stream);

/* ---- round delivery (usn_deliver_round.hip): one ring per endpoint for the
 * up to USN_ROUND_MAX rings of a poll round.  Two launches, whatever count is:
 *   rdeliver_plan_kernel  one workgroup: per (endpoint id, ring) the slots of
 *                         that segment, summed id-major / ring-minor (seg_off,
 *                         ep_off), the header, and the tile prefix over the
 *                         receivers' ROUND rings
 *   rdeliver_pack_kernel  device-sized grid; a tile is USN_DELIVER_TILE slots
 *                         of one receiver's round ring and may span segments:
 *                         per intersected segment the three-list cut at the
 *                         segment-local position, all their runs merged in LDS
 *                         with the ring of every slot, then one gather
 * The per-ring fields are arrays of USN_ROUND_MAX; entries from count on
 * repeat ring 0 with n = 0, so the kernels treat all eight alike (no branch on
 * count) and every position they clamp to n gives an empty list. */
struct RoundDeliverArgs {
  const uint8_t *frames[USN_ROUND_MAX];
  uint64_t stride[USN_ROUND_MAX];
  const uint64_t *offsets[USN_ROUND_MAX];
  const uint16_t *lens[USN_ROUND_MAX];
  const uint32_t *index[USN_ROUND_MAX];
  const uint32_t *bin_off[USN_ROUND_MAX];
  const usn_summary *summary[USN_ROUND_MAX];
  uint32_t n[USN_ROUND_MAX];     /* frames in ring k (< 2^32 - 1) */
  uint32_t src[USN_ROUND_MAX];   /* ring k's source endpoint */
  const uint16_t *eptab;    /* as DeliverArgs */
  uint8_t *out_frames;
  uint16_t *out_lens;
  uint32_t *out_src;
  uint32_t *ep_off;         /* [USN_DT_IDS] */
  uint32_t *seg_off;        /* [USN_ROUND_MAX * USN_DT_IDS + 1] */
  usn_delivery_hdr *hdr;
  uint32_t *tile_pfx;       /* [USN_DT_IDS], as DeliverArgs, over the round rings */
  uint32_t cap, slot;
};
hipError_t launch_deliver_round(const RoundDeliverArgs &a, uint32_t pack_grid, hipStream_t stream);

/* ---- ring delivery (usn_deliver_rings.hip): a poll round appended to the
 * persistent, circular per-endpoint rings of a usn_ringset.  Three launches,
 * whatever count is:
 *   rings_plan_kernel    one workgroup: per (endpoint id, ring) the offered
 *                        count (the round plan's rule), the id's free space
 *                        from head / tail / ring_off, the tail-drop in
 *                        registers (seg_acc, first, acc, drop), the next tails
 *                        (scratch), the header, and the tile prefix over the
 *                        receivers' ACCEPTED runs
 *   rings_pack_kernel    device-sized grid; a tile is USN_DELIVER_TILE
 *                        positions of one receiver's accepted run: the round
 *                        pack's segment cuts and merge bounded by seg_acc, the
 *                        output slot (first + position) & (S - 1) in the ring
 *   rings_commit_kernel  one workgroup: tail[] = the next tails
 * The per-ring fields are RoundDeliverArgs' (entries from count on repeat ring
 * 0 with n = 0). */
struct RingsDeliverArgs {
  const uint8_t *frames[USN_ROUND_MAX];
  uint64_t stride[USN_ROUND_MAX];
  const uint64_t *offsets[USN_ROUND_MAX];
  const uint16_t *lens[USN_ROUND_MAX];
  const uint32_t *index[USN_ROUND_MAX];
  const uint32_t *bin_off[USN_ROUND_MAX];
  const usn_summary *summary[USN_ROUND_MAX];
  uint32_t n[USN_ROUND_MAX];
  uint32_t src[USN_ROUND_MAX];
  const uint16_t *eptab;     /* as DeliverArgs */
  uint8_t *out_frames;       /* the ring set's arrays: total slots */
  uint16_t *out_lens;
  uint32_t *out_src;
  const uint32_t *ring_off;  /* [USN_DT_IDS + 1] */
  const uint32_t *head;      /* [USN_DT_IDS] */
  uint32_t *tail;            /* [USN_DT_IDS]: read by the plan, written by the commit */
  uint32_t *first, *acc, *drop;   /* [USN_DT_IDS] each */
  uint32_t *seg_acc;         /* [USN_ROUND_MAX * USN_DT_IDS] */
  usn_ringset_hdr *hdr;
  uint32_t *tile_pfx;        /* [USN_DT_IDS]: tiles of the accepted runs of the ids below */
  uint32_t *next_tail;       /* [USN_DT_IDS]: first + acc, until the commit */
  uint32_t total, slot;
};
/* scratch behind usn_ringset.hdr, from DELIVER_SCRATCH_OFF: tile_pfx, next_tail */
constexpr size_t RINGS_SCRATCH_BYTES = 2 * DELIVER_SCRATCH_BYTES;
hipError_t launch_deliver_rings(const RingsDeliverArgs &a, uint32_t pack_grid, hipStream_t stream);

/* ---- ring drain (usn_rings_drain.hip): the consumer of a usn_ringset.  Up to
 * budget[e] of ring e's oldest frames, ids ascending, byte-compact in
 * usn_deliver_packed's layout, and the heads moved.  Four launches:
 *   drain_plan_kernel  one workgroup: avail / want per id from ring_off, head,
 *                      tail and budget, the capacity handed out in id order
 *                      (from, take, left, ep_off), the next heads (scratch),
 *                      the header, and the tile prefix over the selected runs
 *   drain_sum_kernel   device-sized grid: per tile its ring slots' lens read
 *                      coalesced, the 16-byte pieces (sum of ceil16(min(len,
 *                      slot)) / 16) into tile_b16[t]
 *   drain_scan_kernel  one workgroup: the packed scan (tile_base, ep_boff,
 *                      need_bytes, the byte-overflow flag) and, when the call
 *                      fits, the commit: head[] = the next heads
 *   drain_copy_kernel  device-sized grid: per tile lens / src read from the
 *                      ring, the pieces' scan in LDS, off16 / lens / src, and
 *                      the output-stationary gather out of the ring slots */
struct DrainArgs {
  const uint8_t *frames;     /* the ring set's arrays: total slots, read only */
  const uint16_t *lens;
  const uint32_t *src;
  const uint32_t *ring_off;  /* [USN_DT_IDS + 1] */
  uint32_t *head;            /* [USN_DT_IDS]: read by the plan, written by the scan's commit */
  const uint32_t *tail;      /* [USN_DT_IDS] */
  uint8_t *out_frames;
  uint32_t *out_off16;
  uint16_t *out_lens;
  uint32_t *out_src;
  uint32_t *ep_off;          /* [USN_DT_IDS + 1] */
  uint64_t *ep_boff;         /* [USN_DT_IDS + 1] */
  const uint32_t *budget;    /* [USN_DT_IDS] */
  uint32_t *from, *take, *left;   /* [USN_DT_IDS] each */
  usn_drain_hdr *hdr;
  uint32_t *tile_pfx;        /* [USN_DT_IDS]: tiles of the selected runs of the ids below */
  uint32_t *next_head;       /* [USN_DT_IDS]: from + take, until the commit */
  uint64_t *tile_base;       /* [max tiles]: 16-byte pieces before tile t */
  uint32_t *tile_b16;        /* [max tiles]: 16-byte pieces of tile t */
  uint32_t total, slot;      /* the ring set's */
  uint32_t cap;
  uint64_t cap_bytes;
};
/* scratch behind usn_drain.hdr, from DELIVER_SCRATCH_OFF: tile_pfx, next_head,
 * then tile_base and tile_b16 for pdeliver_max_tiles(cap) tiles */
constexpr size_t DRAIN_BASE_OFF = DELIVER_SCRATCH_OFF + 2 * DELIVER_SCRATCH_BYTES;   /* 8-byte aligned */
constexpr size_t drain_scratch_bytes(uint64_t cap) {
  return 2 * DELIVER_SCRATCH_BYTES + pdeliver_max_tiles(cap) * 12;
}
hipError_t launch_rings_drain(const DrainArgs &a, uint32_t grid, hipStream_t stream);

/* ---- byte-ring delivery (usn_deliver_brings.hip): a poll round appended to
 * the persistent, byte-compact rings of a usn_bringset.  Five launches,
 * whatever count is:
 *   brings_plan_kernel    one workgroup: the ring plan's counting, the id's
 *                         free descriptors and free units (head, tail, btail
 *                         and pos16 at the head descriptor), the descriptor-
 *                         bounded acceptance per segment (seg_d), first /
 *                         bfirst, the offered count per id and the tile prefix
 *                         over the descriptor-bounded runs
 *   brings_merge_kernel   device-sized grid: the ring pack's segment cuts and
 *                         merge per tile; src / lens into the staging area,
 *                         the tile's units into tile_u[t]; no frame byte moves
 *   brings_scan_kernel    one workgroup: exclusive scan of tile_u restarted at
 *                         every receiver's first tile (tile_base)
 *   brings_copy_kernel    device-sized grid: a tile behind the byte cut leaves
 *                         at once; else the units' scan in LDS, the cut at
 *                         free_u, the descriptors, the output-stationary gather
 *                         into the wrapped byte ring, and one tile per run
 *                         notes the run's accepted frames and units
 *   brings_commit_kernel  one workgroup: acc, drop, acc_units, seg_acc, the
 *                         header, tail and btail
 * The per-ring fields are RoundDeliverArgs'. */
struct BRingsDeliverArgs {
  const uint8_t *frames[USN_ROUND_MAX];
  uint64_t stride[USN_ROUND_MAX];
  const uint64_t *offsets[USN_ROUND_MAX];
  const uint16_t *lens[USN_ROUND_MAX];
  const uint32_t *index[USN_ROUND_MAX];
  const uint32_t *bin_off[USN_ROUND_MAX];
  const usn_summary *summary[USN_ROUND_MAX];
  uint32_t n[USN_ROUND_MAX];
  uint32_t src[USN_ROUND_MAX];
  const uint16_t *eptab;     /* as DeliverArgs */
  uint8_t *out_frames;       /* the set's arrays: total_units units, total_desc descriptors */
  uint16_t *out_lens;
  uint32_t *out_src;
  uint32_t *out_pos16;
  const uint32_t *desc_off;  /* [USN_DT_IDS + 1] */
  const uint32_t *unit_off;  /* [USN_DT_IDS + 1] */
  const uint32_t *head;      /* [USN_DT_IDS] */
  uint32_t *tail, *btail;    /* [USN_DT_IDS]: read by the plan, moved by the commit */
  uint32_t *first, *bfirst, *acc, *drop, *acc_units;   /* [USN_DT_IDS] each */
  uint32_t *seg_acc;         /* [USN_ROUND_MAX * USN_DT_IDS] */
  usn_bringset_hdr *hdr;
  /* scratch */
  uint32_t *tile_pfx;        /* [USN_DT_IDS]: tiles of the descriptor-bounded runs of the ids below */
  uint32_t *free_u;          /* [USN_DT_IDS]: free units before the call */
  uint32_t *run_acc;         /* [USN_DT_IDS]: a run's accepted frames, by its one deciding tile */
  uint32_t *run_units;       /* [USN_DT_IDS]: ... and units */
  uint32_t *seg_d;           /* [USN_ROUND_MAX * USN_DT_IDS]: segment (e, k)'s share of the first free_d frames */
  uint64_t *offered;         /* [USN_DT_IDS]: frames offered to the id */
  uint32_t *st_src;          /* [total_desc]: the run of id e at desc_off[e], unwrapped */
  uint16_t *st_lens;         /* [total_desc] */
  uint32_t *tile_u;          /* [max_tiles]: units of tile t */
  uint32_t *tile_first;      /* [max_tiles]: first tile of t's run */
  uint32_t *tile_base;       /* [max_tiles]: units before tile t in its run (saturating) */
  uint32_t total_desc, total_units, max_tiles;
};
/* the most tiles a call has: a receiver's last tile may be short */
constexpr size_t brings_max_tiles(uint64_t total_desc) {
  return (size_t)(total_desc / USN_DELIVER_TILE) + USN_DT_IDS + 1;
}
/* scratch behind usn_bringset.hdr, from DELIVER_SCRATCH_OFF: the per-id part
 * (tile_pfx, free_u, run_acc, run_units, seg_d, offered), then st_src, st_lens
 * (each rounded up to 16 bytes) and tile_u, tile_first, tile_base */
constexpr size_t BRINGS_IDS_BYTES = (size_t)USN_DT_IDS * (4 * 4 + 4 * USN_ROUND_MAX + 8);
constexpr size_t brings_scratch_bytes(uint64_t total_desc) {
  return BRINGS_IDS_BYTES + (((size_t)total_desc * 4 + 15) & ~(size_t)15) +
         (((size_t)total_desc * 2 + 15) & ~(size_t)15) + 3 * ((brings_max_tiles(total_desc) * 4 + 15) & ~(size_t)15);
}
hipError_t launch_deliver_brings(const BRingsDeliverArgs &a, uint32_t grid, hipStream_t stream);

/* ---- byte-ring drain (usn_brings_drain.hip): the consumer of a usn_bringset,
 * into the ring drain's region (usn_drain).  The queued bytes of a byte ring
 * are compact already, so nothing is summed or scanned per tile.  Three
 * launches:
 *   bdrain_plan_kernel    one workgroup: avail / want per id from desc_off,
 *                         unit_off, head, tail, btail, budget and pos16 at the
 *                         head descriptor, the ring drain's selection (from,
 *                         take, left, ep_off), the units of every run from one
 *                         more pos16 read (ep_boff, need_bytes, the overflow
 *                         decision), the header, and two tile prefixes: over
 *                         the selected descriptors and over the runs' units
 *   bdrain_copy_kernel    device-sized grid: descriptor tiles (lens / src read
 *                         from the ring, off16 from pos16, the chain check),
 *                         then unit tiles (USN_BDRAIN_UTILE units of one run,
 *                         copied unit for unit out of the wrapped byte ring)
 *   bdrain_commit_kernel  one workgroup: unless bytes overflowed or a chain
 *                         broke, head[] = from + take and taken = selected */
struct BDrainArgs {
  const uint8_t *frames;     /* the set's arrays: total_units units, total_desc descriptors, read only */
  const uint16_t *lens;
  const uint32_t *src;
  const uint32_t *pos16;
  const uint32_t *desc_off;  /* [USN_DT_IDS + 1] */
  const uint32_t *unit_off;  /* [USN_DT_IDS + 1] */
  uint32_t *head;            /* [USN_DT_IDS]: read by the plan, written by the commit */
  const uint32_t *tail, *btail;   /* [USN_DT_IDS] */
  uint8_t *out_frames;
  uint32_t *out_off16;
  uint16_t *out_lens;
  uint32_t *out_src;
  uint32_t *ep_off;          /* [USN_DT_IDS + 1] */
  uint64_t *ep_boff;         /* [USN_DT_IDS + 1] */
  const uint32_t *budget;    /* [USN_DT_IDS] */
  uint32_t *from, *take, *left;   /* [USN_DT_IDS] each */
  usn_drain_hdr *hdr;
  /* scratch behind usn_drain.hdr, inside drain_scratch_bytes: the ring drain's tile_pfx and
   * next_head places, and the first USN_DT_IDS words at DRAIN_BASE_OFF (12 * USN_DT_IDS bytes
   * are there whatever cap is) */
  uint32_t *dtile_pfx;       /* [USN_DT_IDS]: descriptor tiles of the selected runs of the ids below */
  uint32_t *utile_pfx;       /* [USN_DT_IDS]: unit tiles of the runs of the ids below; all 0 on byte overflow */
  uint32_t *p0;              /* [USN_DT_IDS]: pos16 at the head descriptor */
  uint32_t total_desc, total_units;
  uint32_t cap;
  uint64_t cap_bytes;
};
static_assert(pdeliver_max_tiles(1) * 12 >= (size_t)USN_DT_IDS * 4, "p0 fits the drain's tile scratch");
hipError_t launch_brings_drain(const BDrainArgs &a, uint32_t grid, hipStream_t stream);

}  // namespace usn

/* the same kernels at 512 threads per tile (a second compilation of
 * usn_device.hip); usn_host.cpp use_t512() picks the build per launch */
namespace usn_t512 {
hipError_t launch_classify(const usn::MultiArgs &m, hipStream_t stream);
/* done (optional): an event bound to the scatter kernel's dispatch, complete
 * when the lists are (hipExtLaunchKernel's stop event) */
hipError_t launch_scatter(const usn::ScatterArgs &s, hipStream_t stream, hipEvent_t done = nullptr);
uint32_t scatter_fallbacks();   /* chunks the scatter ranked again (current device) */
hipError_t launch_tx(const usn::TxArgs &t, hipStream_t stream);
bool table_fits_lds(uint32_t nbins, uint32_t table_units);
}

#endif
