/*
 * usn_deliver_rings.hip -- a poll round appended to persistent, circular
 * per-endpoint rings (usn_deliver_rings; gfx950).
 *
 * An endpoint of the reference owns one ring of fixed size; a write into a
 * full ring fails and that frame alone is lost (src/endpoint.rs:75-82).  Within
 * one poll round nothing is consumed, so of what the round offers endpoint e
 * (usn_deliver_round's round ring: segment (e, 0), then (e, 1), ...) the first
 * `free` frames are accepted and the rest dropped.  A usn_ringset holds those
 * rings in HBM: ring e = slots [ring_off[e], ring_off[e + 1]), a power of two
 * S of them, free-running head / tail, slot of position p = p & (S - 1).
 *
 * Work split, three launches whatever the round's ring count is.
 *
 * Plan (one workgroup): the round plan's counting -- a thread owns four ids
 * and all eight rings of each, every bin_off load in flight together -- plus
 * the ids' ring_off, head and tail.  The tail-drop is local to an id and runs
 * in registers (left = free; a = min(cnt, left); left -= a), no exchange
 * between threads; what crosses threads is one scan (tiles of the ACCEPTED
 * runs) and the totals.  There is no overflow branch: an id without room just
 * has no tile.
 *
 * Pack (device-sized grid): a tile is USN_DELIVER_TILE consecutive positions
 * of one receiver's accepted run.  Wave 0 prefixes the receiver's eight
 * seg_acc with wave shuffles and, for every accepted segment the tile
 * intersects, cuts that ring's three lists at the segment-local position
 * (lists_cut); the count after the cut is bounded by the ACCEPTED count, so a
 * truncated segment ends mid-list and nothing of a dropped frame is read.  The
 * runs side by side in LDS, the one-pass merge, the plain-tile shortcut and the
 * frame address from the ring table in LDS are usn_deliver_round.hip's.  The
 * destination is new: position j of the run goes to slot base + ((first + j) &
 * (S - 1)), formed from four scalars where it is used (the src[] / lens[] pass
 * and the gather), never stored per slot.  An accepted run never exceeds its
 * ring, so a tile crosses the wrap at most once and its stores are two
 * contiguous spans.
 *
 * Commit (one workgroup): tail[] = first + acc, after every slot is written.
 *
 * Every index is clamped: list positions to n, ring_off to total, the output
 * slot to its ring -- whatever lists, heads, tails or ring_off hold, no access
 * leaves the result, the batch or the ring set.
 */
#include "usn_deliver_common.h"

namespace usn {
namespace {

using namespace dv;
constexpr uint32_t UNR = 4;                  // frames a lane group has in flight
constexpr uint32_t RM = USN_ROUND_MAX;
static_assert(RM == 8 && RM + 1 <= 64, "a receiver's segment counts: one lane each, 8e + k");

/* what wave 0 hands the workgroup per tile */
enum { T_M = 0, T_W0 = 1, T_NS = 2, T_PLAIN = 3, T_BASE = 4, T_MASK = 5, T_WORDS = 6 };

__global__ __launch_bounds__(PLAN_T) void rings_plan_kernel(RingsDeliverArgs a) {
  __shared__ unsigned long long wsum[PLAN_T / 64];
  __shared__ uint32_t s_recv;
  const uint32_t tid = threadIdx.x, e0 = tid * 4;
  if (tid == 0) s_recv = 0;
  /* as the round plan: per ring n_ep and for_nic(src) (uniform), then every
   * bin_off entry this thread needs, and with them its ids' ring_off (five),
   * head and tail -- all issued before the first is used */
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
  const u32x4 ro4 = *reinterpret_cast<const u32x4 *>(a.ring_off + e0);
  const uint32_t ro_end = a.ring_off[e0 + 4];
  const u32x4 hd = *reinterpret_cast<const u32x4 *>(a.head + e0);
  const u32x4 tl = *reinterpret_cast<const u32x4 *>(a.tail + e0);
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
  /* the tail-drop, id by id in registers */
  uint32_t ro[5] = {ro4.x, ro4.y, ro4.z, ro4.w, ro_end};
#pragma unroll
  for (uint32_t j = 0; j < 5; ++j) ro[j] = ro[j] < a.total ? ro[j] : a.total;
  const uint32_t head[4] = {hd.x, hd.y, hd.z, hd.w}, tail[4] = {tl.x, tl.y, tl.z, tl.w};
  uint32_t acc[4], drop[4], tlj[4];
  unsigned long long tiles_t = 0, acc_t = 0, off_t = 0;
  uint32_t recv = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t S = ro[j + 1] > ro[j] ? ro[j + 1] - ro[j] : 0u;
    const uint32_t fill = tail[j] - head[j];            // free-running: a head ahead of the tail fills the ring
    const uint32_t free_ = S - (fill < S ? fill : S);
    uint32_t left = free_, sa[RM], lo = 0, hi = 0;       // the offered sum in 64 bits by hand
#pragma unroll
    for (uint32_t k = 0; k < RM; ++k) {
      sa[k] = cnt[j][k] < left ? cnt[j][k] : left;
      left -= sa[k];
      lo += cnt[j][k];
      hi += lo < cnt[j][k];
    }
    const unsigned long long offered = (unsigned long long)hi << 32 | lo;   // < 2^35
    acc[j] = free_ - left;
    drop[j] = sat32(offered - acc[j]);
    tlj[j] = (acc[j] + P - 1) / P;                       // acc <= S (<= 2^30 as usn_ringset_init lays rings out)
    tiles_t += tlj[j];
    acc_t += acc[j];
    off_t += offered;
    recv += acc[j] != 0;
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.seg_acc + (size_t)(e0 + j) * RM);   // 32-byte aligned
    dst[0] = u32x4{sa[0], sa[1], sa[2], sa[3]};
    dst[1] = u32x4{sa[4], sa[5], sa[6], sa[7]};
  }
  unsigned long long tiles = 0, accepted = 0, offered = 0;
  const uint32_t tp = (uint32_t)plan_scan(tiles_t, wsum, &tiles);
  plan_scan(acc_t, wsum, &accepted);
  plan_scan(off_t, wsum, &offered);
  if (recv) atomicAdd(&s_recv, recv);
  *reinterpret_cast<u32x4 *>(a.tile_pfx + e0) = u32x4{tp, tp + tlj[0], tp + tlj[0] + tlj[1], tp + tlj[0] + tlj[1] + tlj[2]};
  *reinterpret_cast<u32x4 *>(a.first + e0) = tl;
  *reinterpret_cast<u32x4 *>(a.acc + e0) = u32x4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<u32x4 *>(a.drop + e0) = u32x4{drop[0], drop[1], drop[2], drop[3]};
  *reinterpret_cast<u32x4 *>(a.next_tail + e0) =
      u32x4{tail[0] + acc[0], tail[1] + acc[1], tail[2] + acc[2], tail[3] + acc[3]};
  __syncthreads();
  if (tid == 0) {
    a.hdr->offered = offered;
    a.hdr->dropped = offered - accepted;
    a.hdr->accepted = sat32(accepted);
    a.hdr->n_recv = s_recv;
    a.hdr->flags = offered != accepted ? USN_DV_DROPPED : 0u;   // the pack ORs USN_DV_LONG in
    a.hdr->_r = 0;
  }
}

__global__ __launch_bounds__(PACK_T) void rings_pack_kernel(RingsDeliverArgs a) {
  __shared__ uint32_t s_run[3][P];
  __shared__ uint32_t s_src[P];
  __shared__ uint16_t s_len[P];
  __shared__ uint8_t s_rb[P];               // the source ring of the tile's position
  __shared__ uint64_t s_addr[P];            // the address of its frame
  __shared__ uint32_t s_seg[RM][S_WORDS];
  __shared__ uint32_t s_h[T_WORDS];
  /* the ring table */
  __shared__ const uint8_t *t_frames[RM];
  __shared__ uint64_t t_stride[RM];
  __shared__ const uint64_t *t_offsets[RM];
  __shared__ const uint16_t *t_lens[RM];
  __shared__ const uint32_t *t_index[RM];
  __shared__ const uint32_t *t_bin_off[RM];
  __shared__ uint32_t t_n[RM], t_src[RM], t_n_ep[RM], t_nic[RM];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // stream order makes the plan's prefix, seg_acc and first visible
  const uint32_t ntile = a.tile_pfx[USN_DT_IDS - 1];   // the last id is never registered: the tile total
  if (blockIdx.x >= ntile) return;
#pragma unroll
  for (uint32_t k = 0; k < RM; ++k)
    if (tid == k) {
      t_frames[k] = a.frames[k];
      t_stride[k] = a.stride[k];
      t_offsets[k] = a.offsets[k];
      t_lens[k] = a.lens[k];
      t_index[k] = a.index[k];
      t_bin_off[k] = a.bin_off[k];
      t_n[k] = a.n[k];   // 0 from count on: nothing is read through such a ring
      t_src[k] = a.src[k];
      const uint32_t v = a.summary[k]->n_ep;
      t_n_ep[k] = v < USN_MAX_ENDPOINTS ? v : USN_MAX_ENDPOINTS;
      t_nic[k] = a.eptab[a.src[k]];
    }
  const uint32_t pieces = a.slot >> 4;
  const uint32_t g = pieces < 64u ? pieces : 64u;   // lanes per frame
  const uint32_t fpw = 64u / g;                     // frames per wave and pass
  const uint32_t lgrp = lane / g, sub = lane - lgrp * g;
  const uint32_t ngroups = (PACK_T / 64u) * fpw, gid = wave * fpw + lgrp;
  __syncthreads();

  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    if (wave == 0) {
      const uint32_t e = tile_receiver(a.tile_pfx, t, lane);
      const uint32_t k0 = (t - a.tile_pfx[e]) * P;   // in the accepted run; < its length
      /* lane k: the accepted frames of the segments before k (lane RM: of all) */
      const uint32_t sa = lane < RM ? a.seg_acc[(size_t)e * RM + lane] : 0u;
      uint32_t inc = sa;
      for (uint32_t d = 1; d <= RM; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
      }
      const uint32_t rel = inc - sa;
      /* the ring: clamped to the set, so a slot below base + S lies inside it */
      uint32_t base = a.ring_off[e], end = a.ring_off[e + 1];
      base = base < a.total ? base : a.total;
      end = end < a.total ? end : a.total;
      const uint32_t S = end > base ? end - base : 0u;
      uint32_t total = __builtin_amdgcn_readlane(rel, RM);   // readlane: the tile's bounds stay scalar
      total = total < S ? total : S;                 // an accepted run never exceeds its ring
      const uint32_t m = k0 < total ? (total - k0 < P ? total - k0 : P) : 0u;
      uint32_t ns = 0;
      bool plain = true;   // every intersected segment continues one list only
      for (uint32_t k = 0; k < RM; ++k) {
        const uint32_t s0 = __builtin_amdgcn_readlane(rel, k), s1 = __builtin_amdgcn_readlane(rel, k + 1);
        const uint32_t b0 = s0 > k0 ? s0 : k0, b1 = s1 < k0 + m ? s1 : k0 + m;
        if (b0 >= b1) continue;                      // the tile holds nothing accepted of segment k
        const RingLists rl{a.eptab, t_bin_off[k], t_src[k], t_n[k]};
        uint32_t lo[3], hi[3], len[3], x[3];
        recv_lists(rl, e, t_n_ep[k], t_nic[k], lo, hi);
        for (int r = 0; r < 3; ++r) len[r] = hi[r] - lo[r];
        const uint32_t ltot = len[0] + len[1] + len[2];   // >= s1 - s0: what was offered
        const uint32_t p = b0 - s0 < ltot ? b0 - s0 : ltot;
        const uint32_t cnt = b1 - b0 < ltot - p ? b1 - b0 : ltot - p;   // ends with the accepted share
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
        s_h[T_W0] = a.first[e] + k0;   // free-running position of the tile's first slot
        s_h[T_NS] = ns;
        s_h[T_PLAIN] = plain;
        s_h[T_BASE] = base;
        s_h[T_MASK] = S - 1u;          // S >= 1 wherever m > 0
      }
    }
    __syncthreads();
    /* the same for every lane: kept scalar, the slot mapping costs the gather no vector register */
    const uint32_t m = s_h[T_M], ns = s_h[T_NS];
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(s_h[T_W0]), base = __builtin_amdgcn_readfirstlane(s_h[T_BASE]),
                   mask = __builtin_amdgcn_readfirstlane(s_h[T_MASK]);
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
       * positions from cnt on belong to the next tile, or to dropped frames */
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
    /* src[] / lens[]: position i of the tile is slot base + ((w0 + i) & mask), two contiguous
     * spans when the tile crosses the wrap */
    bool is_long = false;
    for (uint32_t i = tid; i < m; i += PACK_T) {
      const uint32_t fi = s_src[i], k = s_rb[i] & (RM - 1u);
      const uint16_t ln = fi < t_n[k] ? as_global(t_lens[k])[fi] : (uint16_t)0;
      uint64_t ad = 0;   // where the frame lies: its ring's base, stride or offsets[] from the ring table
      if (ln) {
        const uint64_t st = t_stride[k];
        ad = (uint64_t)t_frames[k] + (st ? (uint64_t)fi * st : as_global(t_offsets[k])[fi]);
      }
      s_addr[i] = ad;
      s_len[i] = ln;   // 0 unless the index lies inside its ring
      const uint32_t o = base + ((w0 + i) & mask);   // < base + S <= total
      a.out_src[o] = fi;
      a.out_lens[o] = ln;
      is_long |= ln > a.slot;
    }
    if (is_long) atomicOr(&a.hdr->flags, USN_DV_LONG);
    __syncthreads();
    /* gather: g lanes per frame, UNR frames' loads in flight per lane */
    if (lgrp < fpw) {
      for (uint32_t f0 = gid; f0 < m; f0 += ngroups * UNR) {
        const USN_GLOBAL uint8_t *sp[UNR];
        uint32_t ln[UNR], maxlen = 0;
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u) {
          const uint32_t f = f0 + u * ngroups;
          ln[u] = 0;
          sp[u] = nullptr;
          if (f < m) {
            const uint32_t l = s_len[f];
            ln[u] = l < a.slot ? l : a.slot;
            sp[u] = (const USN_GLOBAL uint8_t *)s_addr[f];
          }
          maxlen = ln[u] > maxlen ? ln[u] : maxlen;
        }
        for (uint32_t b = sub * 16u; b < maxlen; b += g * 16u) {
          u32x4 v[UNR];
#pragma unroll
          for (uint32_t u = 0; u < UNR; ++u)
            if (b < ln[u]) v[u] = *reinterpret_cast<const USN_GLOBAL u32x4 *>(sp[u] + b);
#pragma unroll
          for (uint32_t u = 0; u < UNR; ++u)
            if (b < ln[u]) {
              const int nb = (int)(ln[u] - b);   // bytes of the frame in this piece (>= 1)
              if (nb < 16) {
                v[u].x &= keep_mask(nb);
                v[u].y &= keep_mask(nb - 4);
                v[u].z &= keep_mask(nb - 8);
                v[u].w &= keep_mask(nb - 12);
              }
              const uint32_t o = base + ((w0 + f0 + u * ngroups) & mask);
              uint8_t *dp = a.out_frames + (uint64_t)o * a.slot + b;
              *reinterpret_cast<u32x4 *>(dp) = v[u];
            }
        }
      }
    }
    __syncthreads();   // the next tile reuses the LDS
  }
}

/* the call's last launch: every slot is written, the tails may show them */
__global__ __launch_bounds__(PLAN_T) void rings_commit_kernel(RingsDeliverArgs a) {
  const uint32_t e0 = threadIdx.x * 4;
  *reinterpret_cast<u32x4 *>(a.tail + e0) = *reinterpret_cast<const u32x4 *>(a.next_tail + e0);
}

}  // namespace

hipError_t launch_deliver_rings(const RingsDeliverArgs &a, uint32_t pack_grid, hipStream_t stream) {
  hipLaunchKernelGGL(rings_plan_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rings_pack_kernel, dim3(pack_grid), dim3(PACK_T), 0, stream, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rings_commit_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  return hipGetLastError();
}

}  // namespace usn
