/*
 * usn_deliver_brings.hip -- a poll round appended to persistent, circular,
 * BYTE-COMPACT per-endpoint rings (usn_deliver_brings; gfx950).
 *
 * usn_deliver_rings.hip gives every queued frame a slot of the largest frame's
 * size; with mixed sizes (64 / 576 / 1500 in 2048-byte slots) such a ring set
 * is mostly holes.  A usn_bringset splits a ring in two: a descriptor ring of D
 * entries (lens, src, pos16) and a byte ring of B 16-byte units, in which the
 * frames lie back to back, each zero-padded to a unit.  A frame is accepted
 * while a descriptor AND its units are free; the first frame that finds
 * neither ends the receiver's run for this call (strict tail-drop, one cut).
 *
 * Where the cut falls depends on the lengths of all frames before it, which
 * only the merged order gives, so the work is split around a scan:
 *
 *   plan    (one workgroup) usn_deliver_rings' plan: four ids per thread, every
 *           load in flight together, plus desc_off / unit_off / btail and one
 *           dependent load per id, pos16 at the head descriptor (the units in
 *           use are btail - that).  The tail-drop by DESCRIPTORS runs in
 *           registers per segment (seg_d); tiles are those of the descriptor-
 *           bounded runs.
 *   merge   (device-sized grid) the ring pack's cuts and one-pass merge per
 *           tile of P positions, bounded by seg_d; lens are read through the
 *           merged src.  src / lens go to a staging area in scratch at
 *           desc_off[e] + position (unwrapped: a run never exceeds D), the
 *           tile's units to tile_u[t].  No frame byte moves.
 *   scan    (one workgroup) exclusive scan of tile_u in blocks of 1024 tiles
 *           with a carry, RESTARTED at every receiver's first tile: base =
 *           G[t] - G[first tile of t's run], the latter from this block's LDS
 *           or, for the one run that entered the block, from a carried scalar.
 *   copy    (device-sized grid, the same tiles) a tile whose base lies at or
 *           behind free_u leaves on a uniform test: dropped frames cost no
 *           byte traffic.  Else the units' scan in LDS (s_off), the cut at
 *           free_u, the accepted frames' descriptors (two contiguous spans
 *           across the wrap) and the OUTPUT-STATIONARY gather of
 *           usn_deliver_packed.hip: lane i takes units i, i + 256, ... of the
 *           tile's accepted unit range, finds the unit's frame in s_off (or by
 *           a shift when the tile has one unit count), four loads in flight
 *           before the first store; the destination unit (bfirst + base + i) &
 *           (B - 1) comes from the tile's scalars.  Exactly one tile per run,
 *           the one that holds the cut or the run's last, notes the run's
 *           accepted frames and units: no atomics.
 *   commit  (one workgroup) acc, drop, acc_units, seg_acc, the header, and the
 *           only writes of tail and btail.
 *
 * Every index is clamped: list positions to n, desc_off / unit_off to the
 * totals, a descriptor to its ring by & (D - 1) and a unit by & (B - 1), tiles
 * to the scratch's tile count -- whatever the counters hold, no access leaves
 * the results, the batches or the set.  Plain C++ vector loads and stores
 * throughout.
 */
#include "usn_deliver_common.h"

namespace usn {
namespace {

using namespace dv;
constexpr uint32_t UNR = 4;                  // units a lane has in flight
constexpr uint32_t RM = USN_ROUND_MAX;
constexpr uint32_t SCAN_T = PLAN_T;          // one tile per thread and pass
static_assert(RM == 8 && RM + 1 <= 64, "a receiver's segment counts: one lane each, 8e + k");
static_assert(P == 2 * PACK_T, "the copy kernel holds two positions of a tile per thread");

/* what wave 0 of the merge hands the workgroup per tile */
enum { T_M = 0, T_ST0 = 1, T_NS = 2, T_PLAIN = 3, T_FIRST = 4, T_WORDS = 5 };

__device__ __forceinline__ uint32_t units_of(uint32_t len) {   // max(1, ceil16(len) / 16)
  const uint32_t u = (len + 15u) >> 4;
  return u ? u : 1u;
}

__device__ __forceinline__ uint32_t tile_count(const BRingsDeliverArgs &a) {
  const uint32_t nt = a.tile_pfx[USN_DT_IDS - 1];   // the last id is never registered: the tile total
  return nt < a.max_tiles ? nt : a.max_tiles;       // always, unless desc_off is not a prefix
}

/* ring [lo, hi) of a prefix array clamped to total: its base and size */
__device__ __forceinline__ void ring_of(const uint32_t *off, uint32_t e, uint32_t total, uint32_t &base,
                                        uint32_t &size) {
  uint32_t b = off[e], x = off[e + 1];
  b = b < total ? b : total;
  x = x < total ? x : total;
  base = b;
  size = x > b ? x - b : 0u;
}

__global__ __launch_bounds__(PLAN_T) void brings_plan_kernel(BRingsDeliverArgs a) {
  __shared__ unsigned long long wsum[PLAN_T / 64];
  const uint32_t tid = threadIdx.x, e0 = tid * 4;
  /* the ring plan's loads, and with them the ids' desc_off and unit_off (five
   * each), head, tail and btail -- all issued before the first is used */
  uint32_t n_ep[RM], nic[RM];
#pragma unroll
  for (uint32_t k = 0; k < RM; ++k) {   // rings from count on: ring 0 again with n = 0, no branch
    const uint32_t v = a.summary[k]->n_ep;
    n_ep[k] = v < USN_MAX_ENDPOINTS ? v : USN_MAX_ENDPOINTS;
    nic[k] = a.eptab[a.src[k]];
  }
  bool reg[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) reg[j] = e0 + j < USN_MAX_ENDPOINTS && a.eptab[e0 + j] != USN_DT_NONE;
  uint32_t own[RM][5], bins[RM][3];
#pragma unroll
  for (uint32_t k = 0; k < RM; ++k) {
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) own[k][j] = a.bin_off[k][e0 + j < n_ep[k] ? e0 + j : n_ep[k]];
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) bins[k][j] = a.bin_off[k][n_ep[k] + j];
  }
  const u32x4 do4 = *reinterpret_cast<const u32x4 *>(a.desc_off + e0);
  const uint32_t do_end = a.desc_off[e0 + 4];
  const u32x4 uo4 = *reinterpret_cast<const u32x4 *>(a.unit_off + e0);
  const uint32_t uo_end = a.unit_off[e0 + 4];
  const u32x4 hd = *reinterpret_cast<const u32x4 *>(a.head + e0);
  const u32x4 tl = *reinterpret_cast<const u32x4 *>(a.tail + e0);
  const u32x4 bt = *reinterpret_cast<const u32x4 *>(a.btail + e0);
  /* the one dependent load per id: where the oldest queued frame starts */
  uint32_t dof[5] = {do4.x, do4.y, do4.z, do4.w, do_end}, uof[5] = {uo4.x, uo4.y, uo4.z, uo4.w, uo_end};
#pragma unroll
  for (uint32_t j = 0; j < 5; ++j) {
    dof[j] = dof[j] < a.total_desc ? dof[j] : a.total_desc;
    uof[j] = uof[j] < a.total_units ? uof[j] : a.total_units;
  }
  const uint32_t head[4] = {hd.x, hd.y, hd.z, hd.w}, tail[4] = {tl.x, tl.y, tl.z, tl.w},
                 btail[4] = {bt.x, bt.y, bt.z, bt.w};
  uint32_t D[4], B[4], p16[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    D[j] = dof[j + 1] > dof[j] ? dof[j + 1] - dof[j] : 0u;
    B[j] = uof[j + 1] > uof[j] ? uof[j + 1] - uof[j] : 0u;
    p16[j] = D[j] ? a.out_pos16[dof[j] + (head[j] & (D[j] - 1u))] : 0u;   // < dof[j] + D <= total_desc
  }
  /* recv_lists' rule and clamps, per ring (the round plan's) */
  uint32_t cnt[4][RM];
#pragma unroll
  for (uint32_t k = 0; k < RM; ++k) {
    const uint32_t n = a.n[k];
    uint32_t o[5], q[3];
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) o[j] = own[k][j] < n ? own[k][j] : n;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) q[j] = bins[k][j] < n ? bins[k][j] : n;
    const uint32_t n_nic = q[1] > q[0] ? q[1] - q[0] : 0u, n_flood = q[2] > q[1] ? q[2] - q[1] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t e = e0 + j;
      uint32_t v = o[j + 1] > o[j] ? o[j + 1] - o[j] : 0u;
      v += e == nic[k] ? n_nic : 0u;
      v += e != a.src[k] ? n_flood : 0u;
      cnt[j][k] = reg[j] ? v : 0u;   // disjoint lists: <= n
    }
  }
  /* the tail-drop by descriptors, id by id in registers; the byte cut follows in the copy */
  uint32_t fu[4], tlj[4], olo[4], ohi[4];
  unsigned long long tiles_t = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t fill = tail[j] - head[j];              // free-running: a head ahead of the tail fills the ring
    const uint32_t free_d = D[j] - (fill < D[j] ? fill : D[j]);
    const uint32_t used = fill ? btail[j] - p16[j] : 0u;
    fu[j] = B[j] - (used < B[j] ? used : B[j]);
    uint32_t left = free_d, sd[RM], lo = 0, hi = 0;        // the offered sum in 64 bits by hand
#pragma unroll
    for (uint32_t k = 0; k < RM; ++k) {
      sd[k] = cnt[j][k] < left ? cnt[j][k] : left;
      left -= sd[k];
      lo += cnt[j][k];
      hi += lo < cnt[j][k];
    }
    olo[j] = lo;
    ohi[j] = hi;
    tlj[j] = (free_d - left + P - 1) / P;                  // a run of at most D <= 2^30 frames
    tiles_t += tlj[j];
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.seg_d + (size_t)(e0 + j) * RM);   // 32-byte aligned
    dst[0] = u32x4{sd[0], sd[1], sd[2], sd[3]};
    dst[1] = u32x4{sd[4], sd[5], sd[6], sd[7]};
  }
  unsigned long long tiles = 0;
  const uint32_t tp = (uint32_t)plan_scan(tiles_t, wsum, &tiles);
  *reinterpret_cast<u32x4 *>(a.tile_pfx + e0) = u32x4{tp, tp + tlj[0], tp + tlj[0] + tlj[1], tp + tlj[0] + tlj[1] + tlj[2]};
  *reinterpret_cast<u32x4 *>(a.first + e0) = tl;
  *reinterpret_cast<u32x4 *>(a.bfirst + e0) = bt;
  *reinterpret_cast<u32x4 *>(a.free_u + e0) = u32x4{fu[0], fu[1], fu[2], fu[3]};
  u32x4 *off = reinterpret_cast<u32x4 *>(a.offered + e0);   // four 64-bit counts
  off[0] = u32x4{olo[0], ohi[0], olo[1], ohi[1]};
  off[1] = u32x4{olo[2], ohi[2], olo[3], ohi[3]};
}

__global__ __launch_bounds__(PACK_T) void brings_merge_kernel(BRingsDeliverArgs a) {
  __shared__ uint32_t s_run[3][P];
  __shared__ uint32_t s_src[P];
  __shared__ uint8_t s_rb[P];               // the source ring of the tile's position
  __shared__ uint32_t s_seg[RM][S_WORDS];
  __shared__ uint32_t s_h[T_WORDS];
  __shared__ uint32_t s_w[PACK_T / 64];
  /* the ring table */
  __shared__ const uint16_t *t_lens[RM];
  __shared__ const uint32_t *t_index[RM];
  __shared__ const uint32_t *t_bin_off[RM];
  __shared__ uint32_t t_n[RM], t_src[RM], t_n_ep[RM], t_nic[RM];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // stream order makes the plan's prefix and seg_d visible
  const uint32_t ntile = tile_count(a);
  if (blockIdx.x >= ntile) return;
#pragma unroll
  for (uint32_t k = 0; k < RM; ++k)
    if (tid == k) {
      t_lens[k] = a.lens[k];
      t_index[k] = a.index[k];
      t_bin_off[k] = a.bin_off[k];
      t_n[k] = a.n[k];   // 0 from count on: nothing is read through such a ring
      t_src[k] = a.src[k];
      const uint32_t v = a.summary[k]->n_ep;
      t_n_ep[k] = v < USN_MAX_ENDPOINTS ? v : USN_MAX_ENDPOINTS;
      t_nic[k] = a.eptab[a.src[k]];
    }
  __syncthreads();

  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    if (wave == 0) {
      const uint32_t e = tile_receiver(a.tile_pfx, t, lane);
      const uint32_t tp = a.tile_pfx[e];
      const uint32_t k0 = (t - tp) * P;   // in the descriptor-bounded run; < its length
      /* lane k: the run's frames of the segments before k (lane RM: of all) */
      const uint32_t sd = lane < RM ? a.seg_d[(size_t)e * RM + lane] : 0u;
      uint32_t inc = sd;
      for (uint32_t d = 1; d <= RM; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
      }
      const uint32_t rel = inc - sd;
      uint32_t dbase, D;
      ring_of(a.desc_off, e, a.total_desc, dbase, D);
      uint32_t total = __builtin_amdgcn_readlane(rel, RM);   // readlane: the tile's bounds stay scalar
      total = total < D ? total : D;                 // a run never exceeds its descriptor ring
      const uint32_t m = k0 < total ? (total - k0 < P ? total - k0 : P) : 0u;
      uint32_t ns = 0;
      bool plain = true;   // every intersected segment continues one list only
      for (uint32_t k = 0; k < RM; ++k) {
        const uint32_t s0 = __builtin_amdgcn_readlane(rel, k), s1 = __builtin_amdgcn_readlane(rel, k + 1);
        const uint32_t b0 = s0 > k0 ? s0 : k0, b1 = s1 < k0 + m ? s1 : k0 + m;
        if (b0 >= b1) continue;                      // the tile holds nothing of segment k
        const RingLists rl{a.eptab, t_bin_off[k], t_src[k], t_n[k]};
        uint32_t lo[3], hi[3], len[3], x[3];
        recv_lists(rl, e, t_n_ep[k], t_nic[k], lo, hi);
        for (int r = 0; r < 3; ++r) len[r] = hi[r] - lo[r];
        const uint32_t ltot = len[0] + len[1] + len[2];   // >= s1 - s0: what was offered
        const uint32_t p = b0 - s0 < ltot ? b0 - s0 : ltot;
        const uint32_t cnt = b1 - b0 < ltot - p ? b1 - b0 : ltot - p;   // ends with the segment's share
        lists_cut(t_index[k], t_n[k], lo, len, p, lane, x);
        uint32_t runs = 0;
        for (int r = 0; r < 3; ++r) runs += x[r] < len[r];
        plain = plain && runs <= 1;
        if (lane == 0) {
          s_seg[ns][S_RING] = k;
          s_seg[ns][S_DST] = b0 - k0;
          s_seg[ns][S_CNT] = cnt;
          for (int r = 0; r < 3; ++r) {
            const uint32_t rem = len[r] - (x[r] < len[r] ? x[r] : len[r]);
            s_seg[ns][S_CUT + r] = lo[r] + x[r];
            s_seg[ns][S_RL + r] = rem < cnt ? rem : cnt;
          }
        }
        ++ns;
      }
      if (lane == 0) {
        s_h[T_M] = m;
        s_h[T_ST0] = dbase + k0;   // staging entry of the tile's first position; + m <= dbase + D
        s_h[T_NS] = ns;
        s_h[T_PLAIN] = plain;
        s_h[T_FIRST] = tp;
      }
    }
    __syncthreads();
    const uint32_t m = s_h[T_M], ns = s_h[T_NS], st0 = s_h[T_ST0], tfirst = s_h[T_FIRST];
    const bool plain = s_h[T_PLAIN] != 0;
    /* every segment's runs, side by side: segment s owns [dst, dst + cnt) of each run array.
     * Where no segment has a second run the one run is the order: straight to
     * s_src, no merge, no barrier */
    for (uint32_t s = 0; s < ns; ++s) {
      const uint32_t dst = s_seg[s][S_DST], cnt = s_seg[s][S_CNT];
      const uint8_t ring = (uint8_t)s_seg[s][S_RING];
      const USN_GLOBAL uint32_t *idx = as_global(t_index[ring]);
      for (int r = 0; r < 3; ++r) {
        const uint32_t cut = s_seg[s][S_CUT + r], rl = s_seg[s][S_RL + r];
        if (plain) {
          for (uint32_t i = tid; i < rl && i < cnt; i += PACK_T) {
            s_src[dst + i] = idx[cut + i];
            s_rb[dst + i] = ring;
          }
        } else {
          for (uint32_t i = tid; i < rl; i += PACK_T) s_run[r][dst + i] = idx[cut + i];
        }
      }
    }
    if (!plain) {
      __syncthreads();
      /* an entry's position: its place in its run plus its rank in the segment's other two;
       * positions from cnt on belong to the next tile, or lie behind the run */
      for (uint32_t s = 0; s < ns; ++s) {
        const uint32_t dst = s_seg[s][S_DST], cnt = s_seg[s][S_CNT];
        const uint8_t ring = (uint8_t)s_seg[s][S_RING];
        uint32_t rl[3];
        for (int r = 0; r < 3; ++r) rl[r] = s_seg[s][S_RL + r];
        for (int r = 0; r < 3; ++r) {
          const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
          for (uint32_t i = tid; i < rl[r]; i += PACK_T) {
            const uint32_t v = s_run[r][dst + i];
            const uint32_t pos =
                i + lbound(s_run[r1] + dst, 0, rl[r1], v) + lbound(s_run[r2] + dst, 0, rl[r2], v);
            if (pos < cnt) {
              s_src[dst + pos] = v;
              s_rb[dst + pos] = ring;
            }
          }
        }
      }
    }
    __syncthreads();
    /* lens through the merged src; both to the staging area, the units summed */
    uint32_t q = 0;   // this thread's units (<= 2 x 4096)
    for (uint32_t i = tid; i < m; i += PACK_T) {
      const uint32_t fi = s_src[i], k = s_rb[i] & (RM - 1u);
      const uint16_t ln = fi < t_n[k] ? as_global(t_lens[k])[fi] : (uint16_t)0;   // 0 unless the index lies inside its ring
      a.st_src[st0 + i] = fi;
      a.st_lens[st0 + i] = ln;
      q += units_of(ln);       // the copy kernel reads exactly these back
    }
    for (uint32_t d = 32; d; d >>= 1) q += __shfl_xor(q, d, 64);
    if (lane == 0) s_w[wave] = q;
    __syncthreads();   // and: the next tile may reuse s_h, s_seg, s_run, s_src
    if (tid == 0) {
      uint32_t tot = 0;
      for (uint32_t k = 0; k < PACK_T / 64; ++k) tot += s_w[k];
      a.tile_u[t] = tot;
      a.tile_first[t] = tfirst;
    }
    // the next tile's write of s_w lies behind its own barriers
  }
}

__global__ __launch_bounds__(SCAN_T) void brings_scan_kernel(BRingsDeliverArgs a) {
  __shared__ unsigned long long wsum[SCAN_T / 64];
  __shared__ unsigned long long s_g[SCAN_T];   // units before the block's tile, over all runs
  const uint32_t tid = threadIdx.x;
  const uint32_t ntile = tile_count(a);
  unsigned long long carry = 0, run_g = 0;     // run_g: units before the first tile of the run that entered the block
  uint32_t v = tid < ntile ? a.tile_u[tid] : 0u;
  uint32_t ft = tid < ntile ? a.tile_first[tid] : 0u;
  for (uint32_t t0 = 0; t0 < ntile; t0 += SCAN_T) {
    // the next block's loads are in flight over this block's scan (t0 + SCAN_T cannot wrap: ntile < 2^24)
    const uint32_t tn = t0 + SCAN_T + tid;
    const uint32_t vn = tn < ntile ? a.tile_u[tn] : 0u;
    const uint32_t ftn = tn < ntile ? a.tile_first[tn] : 0u;
    unsigned long long tot;
    const unsigned long long g = carry + plan_scan(v, wsum, &tot);
    s_g[tid] = g;
    __syncthreads();
    const uint32_t t = t0 + tid;
    if (t < ntile) {
      const uint32_t f = ft < t ? ft : t;   // always: a run's first tile is not behind it
      a.tile_base[t] = sat32(g - (f >= t0 ? s_g[f - t0] : run_g));
    }
    /* the run that leaves the block: that of its last tile */
    const uint32_t tl = (ntile - t0 < SCAN_T ? ntile - t0 : SCAN_T) - 1u;
    uint32_t fl = a.tile_first[t0 + tl];
    fl = fl < t0 + tl ? fl : t0 + tl;
    if (fl >= t0) run_g = s_g[fl - t0];
    __syncthreads();   // s_g is written again by the next block
    carry += tot;
    v = vn;
    ft = ftn;
  }
}

__global__ __launch_bounds__(PACK_T) void brings_copy_kernel(BRingsDeliverArgs a) {
  __shared__ uint32_t s_off[P + 1];   // units before frame i of the tile; [m .. P] = the tile's total
  __shared__ uint64_t s_addr[P];      // the address of frame i
  __shared__ uint16_t s_len[P];
  __shared__ uint32_t s_w[2][PACK_T / 64];
  __shared__ uint32_t s_q0, s_mixed;
  /* the ring table */
  __shared__ const uint8_t *t_frames[RM];
  __shared__ uint64_t t_stride[RM];
  __shared__ const uint64_t *t_offsets[RM];
  __shared__ uint32_t t_n[RM];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // stream order makes the plan's, the merge's and the scan's scratch visible
  const uint32_t ntile = tile_count(a);
  if (blockIdx.x >= ntile) return;
#pragma unroll
  for (uint32_t k = 0; k < RM; ++k)
    if (tid == k) {
      t_frames[k] = a.frames[k];
      t_stride[k] = a.stride[k];
      t_offsets[k] = a.offsets[k];
      t_n[k] = a.n[k];
    }
  __syncthreads();

  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    /* every wave looks the receiver up for itself (two cached loads per lane):
     * no LDS and no barrier for it */
    uint32_t e = tile_receiver(a.tile_pfx, t, lane);
    e = e < USN_MAX_ENDPOINTS ? e : USN_MAX_ENDPOINTS - 1u;   // always: the last id has no tile
    const uint32_t k0 = (t - a.tile_pfx[e]) * P;
    const uint32_t base_u = a.tile_base[t], fu = a.free_u[e];
    if (base_u >= fu) {   // behind the byte cut: the same for the whole workgroup, nothing is read
      if (base_u == fu && tid == 0) {   // the cut fell on this tile's start: it speaks for the run
        a.run_acc[e] = k0;
        a.run_units[e] = base_u;
      }
      continue;
    }
    /* lane k: the run's frames of the segments before k (lane RM: of all) */
    const uint32_t sd = lane < RM ? a.seg_d[(size_t)e * RM + lane] : 0u;
    uint32_t inc0 = sd;
    for (uint32_t d = 1; d <= RM; d <<= 1) {
      const uint32_t o = __shfl_up(inc0, d, 64);
      if (lane >= d) inc0 += o;
    }
    const uint32_t rel = inc0 - sd;
    uint32_t r_end[RM];   // where segment k ends in the run
#pragma unroll
    for (uint32_t k = 0; k < RM; ++k) r_end[k] = __builtin_amdgcn_readlane(rel, k + 1);
    uint32_t dbase, D, ubase, B;
    ring_of(a.desc_off, e, a.total_desc, dbase, D);
    ring_of(a.unit_off, e, a.total_units, ubase, B);
    const uint32_t total = r_end[RM - 1] < D ? r_end[RM - 1] : D;
    const uint32_t m = k0 < total ? (total - k0 < P ? total - k0 : P) : 0u;
    const uint32_t room = fu - base_u;   // >= 1; fu <= B
    /* the same for every lane: kept scalar, the ring mapping costs the gather no vector register */
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(a.first[e] + k0), dmask = __builtin_amdgcn_readfirstlane(D - 1u);
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(a.bfirst[e] + base_u), bmask = __builtin_amdgcn_readfirstlane(B - 1u);
    dbase = __builtin_amdgcn_readfirstlane(dbase);
    ubase = __builtin_amdgcn_readfirstlane(ubase);
    if (tid == 0) s_mixed = 0;
    uint32_t q[2], inc[2], ln[2], fi[2];
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {   // positions tid and tid + PACK_T of the tile
      const uint32_t i = tid + h * PACK_T;
      ln[h] = fi[h] = q[h] = 0;
      if (i < m) {                       // dbase + k0 + i < dbase + D <= total_desc
        ln[h] = a.st_lens[dbase + k0 + i];
        fi[h] = a.st_src[dbase + k0 + i];
        q[h] = units_of(ln[h]);
      }
      inc[h] = q[h];
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc[h], d, 64);
        if (lane >= d) inc[h] += o;
      }
      if (lane == 63) s_w[h][wave] = inc[h];
    }
    if (tid == 0) s_q0 = q[0];
    __syncthreads();
    const uint32_t q0 = s_q0;
    uint32_t before = 0, ex[2];
    bool ok[2];
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t i = tid + h * PACK_T;
      uint32_t wb = before;
      for (uint32_t k = 0; k < PACK_T / 64; ++k) {
        const uint32_t sw = s_w[h][k];
        if (k < wave) wb += sw;
        before += sw;
      }
      ex[h] = wb + inc[h] - q[h];
      s_off[i] = ex[h];
      if (i == P - 1) s_off[P] = ex[h] + q[h];
      if (i < m && q[h] != q0) s_mixed = 1;
      ok[h] = i < m && ex[h] + q[h] <= room;   // the byte cut: monotone, so the accepted frames are a prefix
    }
    const uint32_t c = (uint32_t)__syncthreads_count(ok[0]) + (uint32_t)__syncthreads_count(ok[1]);   // <= m
    /* the accepted frames' descriptors: position i is entry dbase + ((d0 + i) & dmask), two
     * contiguous spans when the tile crosses the wrap; and where each frame lies */
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t i = tid + h * PACK_T;
      uint64_t ad = 0;
      uint32_t l = 0;
      if (ok[h]) {
        const uint32_t o = dbase + ((d0 + i) & dmask);   // < dbase + D <= total_desc
        a.out_lens[o] = (uint16_t)ln[h];
        a.out_src[o] = fi[h];
        a.out_pos16[o] = w0 + ex[h];
        uint32_t k = 0;   // the position's source ring: the segment it lies in
#pragma unroll
        for (uint32_t x = 0; x + 1 < RM; ++x) k += k0 + i >= r_end[x];
        if (ln[h] && fi[h] < t_n[k]) {   // always, once the length is not 0
          const uint64_t st = t_stride[k];
          ad = (uint64_t)t_frames[k] + (st ? (uint64_t)fi[h] * st : as_global(t_offsets[k])[fi[h]]);
          l = ln[h];
        }
      }
      s_addr[i] = ad;
      s_len[i] = (uint16_t)l;   // 0: nothing of this frame is read
    }
    __syncthreads();
    const uint32_t au = s_off[c];   // the tile's accepted units (<= room): [c] holds the total when c == m
    if (tid == 0 && (c < m || k0 + m >= total)) {   // the cut lies in this tile, or the run ends here
      a.run_acc[e] = k0 + c;
      a.run_units[e] = base_u + au;
    }
    const bool mixed = s_mixed != 0;
    const int shift = (q0 & (q0 - 1u)) == 0 ? __ffs((int)q0) - 1 : -1;   // q0 >= 1 when au > 0
    for (uint32_t p0 = tid; p0 < au; p0 += PACK_T * UNR) {
      u32x4 v[UNR];
      int nb[UNR];   // bytes of the frame from the unit's start; <= 0: no piece
#pragma unroll
      for (uint32_t u = 0; u < UNR; ++u) {
        const uint32_t p = p0 + u * PACK_T;
        nb[u] = 0;
        if (p < au) {
          uint32_t f, k;
          if (mixed) {
            /* the last frame whose first unit is <= p: it lies below c (s_off[c] = au > p) */
            f = 0;
#pragma unroll
            for (uint32_t step = P / 2; step; step >>= 1)
              if (s_off[f + step] <= p) f += step;
            k = p - s_off[f];
          } else {
            f = shift >= 0 ? p >> shift : p / q0;
            f = f < P ? f : P - 1u;
            k = p - f * q0;
          }
          nb[u] = (int)s_len[f] - (int)(k * 16u);
          if (nb[u] > 0)
            v[u] = *reinterpret_cast<const USN_GLOBAL u32x4 *>((const USN_GLOBAL uint8_t *)s_addr[f] + (uint64_t)k * 16u);
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < UNR; ++u)
        if (nb[u] > 0) {
          if (nb[u] < 16) {
            v[u].x &= keep_mask(nb[u]);
            v[u].y &= keep_mask(nb[u] - 4);
            v[u].z &= keep_mask(nb[u] - 8);
            v[u].w &= keep_mask(nb[u] - 12);
          }
          const uint32_t du = ubase + ((w0 + p0 + u * PACK_T) & bmask);   // < ubase + B <= total_units
          *reinterpret_cast<u32x4 *>(a.out_frames + (uint64_t)du * 16u) = v[u];
        }
    }
    __syncthreads();   // the next tile reuses the LDS
  }
}

/* the call's last launch: every descriptor and unit is written, the tails may show them */
__global__ __launch_bounds__(PLAN_T) void brings_commit_kernel(BRingsDeliverArgs a) {
  __shared__ unsigned long long wsum[PLAN_T / 64];
  const uint32_t tid = threadIdx.x, e0 = tid * 4;
  const u32x4 ra = *reinterpret_cast<const u32x4 *>(a.run_acc + e0);
  const u32x4 ru = *reinterpret_cast<const u32x4 *>(a.run_units + e0);
  const u32x4 f4 = *reinterpret_cast<const u32x4 *>(a.free_u + e0);
  const u32x4 tl = *reinterpret_cast<const u32x4 *>(a.tail + e0);
  const u32x4 bt = *reinterpret_cast<const u32x4 *>(a.btail + e0);
  const u32x4 *off = reinterpret_cast<const u32x4 *>(a.offered + e0);
  const u32x4 o01 = off[0], o23 = off[1];
  const uint32_t racc[4] = {ra.x, ra.y, ra.z, ra.w}, runits[4] = {ru.x, ru.y, ru.z, ru.w},
                 fu[4] = {f4.x, f4.y, f4.z, f4.w};
  const unsigned long long offered[4] = {(unsigned long long)o01.y << 32 | o01.x, (unsigned long long)o01.w << 32 | o01.z,
                                         (unsigned long long)o23.y << 32 | o23.x, (unsigned long long)o23.w << 32 | o23.z};
  uint32_t acc[4], units[4], drop[4];
  unsigned long long acc_t = 0, unit_t = 0, off_t = 0, recv_t = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {   // an id at a time: its eight shares are loaded where they are used
    const u32x4 *p = reinterpret_cast<const u32x4 *>(a.seg_d + (size_t)(e0 + j) * RM);
    const u32x4 s0 = p[0], s1 = p[1];
    const uint32_t s[RM] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    uint32_t run = 0;   // <= free_d <= D
#pragma unroll
    for (uint32_t k = 0; k < RM; ++k) run += s[k];
    /* an id without a run had no tile: its scratch entries are an earlier call's */
    acc[j] = run ? (racc[j] < run ? racc[j] : run) : 0u;
    units[j] = run ? (runits[j] < fu[j] ? runits[j] : fu[j]) : 0u;   // <= free_u <= B
    if (acc[j] == 0) units[j] = 0;
    uint32_t left = acc[j], sa[RM];
#pragma unroll
    for (uint32_t k = 0; k < RM; ++k) {   // clamp(acc - the shares before k, 0, the share of k)
      sa[k] = s[k] < left ? s[k] : left;
      left -= sa[k];
    }
    drop[j] = sat32(offered[j] - acc[j]);
    acc_t += acc[j];
    unit_t += units[j];
    off_t += offered[j];
    recv_t += acc[j] != 0;
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.seg_acc + (size_t)(e0 + j) * RM);
    dst[0] = u32x4{sa[0], sa[1], sa[2], sa[3]};
    dst[1] = u32x4{sa[4], sa[5], sa[6], sa[7]};
  }
  *reinterpret_cast<u32x4 *>(a.acc + e0) = u32x4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<u32x4 *>(a.drop + e0) = u32x4{drop[0], drop[1], drop[2], drop[3]};
  *reinterpret_cast<u32x4 *>(a.acc_units + e0) = u32x4{units[0], units[1], units[2], units[3]};
  *reinterpret_cast<u32x4 *>(a.tail + e0) = u32x4{tl.x + acc[0], tl.y + acc[1], tl.z + acc[2], tl.w + acc[3]};
  *reinterpret_cast<u32x4 *>(a.btail + e0) = u32x4{bt.x + units[0], bt.y + units[1], bt.z + units[2], bt.w + units[3]};
  unsigned long long accepted = 0, acc_units = 0, all = 0, n_recv = 0;
  plan_scan(acc_t, wsum, &accepted);
  plan_scan(unit_t, wsum, &acc_units);
  plan_scan(off_t, wsum, &all);
  plan_scan(recv_t, wsum, &n_recv);
  if (tid == 0) {
    a.hdr->offered = all;
    a.hdr->dropped = all - accepted;
    a.hdr->accepted_units = acc_units;
    a.hdr->accepted = sat32(accepted);
    a.hdr->n_recv = (uint32_t)n_recv;
    a.hdr->flags = all != accepted ? USN_DV_DROPPED : 0u;
    a.hdr->_r = 0;
  }
}

}  // namespace

hipError_t launch_deliver_brings(const BRingsDeliverArgs &a, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(brings_plan_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(brings_merge_kernel, dim3(grid), dim3(PACK_T), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(brings_scan_kernel, dim3(1), dim3(SCAN_T), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(brings_copy_kernel, dim3(grid), dim3(PACK_T), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(brings_commit_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  return hipGetLastError();
}

}  // namespace usn
