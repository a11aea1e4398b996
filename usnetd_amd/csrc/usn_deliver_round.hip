/*
 * usn_deliver_round.hip -- one output ring per endpoint for a whole poll round
 * (usn_deliver_round; gfx950).
 *
 * The reference drains every readable endpoint in one poll round
 * (src/main.rs:1029-1046) and writes each frame straight into its target's
 * ring (src/endpoint.rs:61-74): after a round endpoint e holds one ring,
 * source 0's frames for it, then source 1's, ...  Here the round is up to
 * USN_ROUND_MAX classified rings; segment (e, k) is what usn_deliver gives
 * receiver e for ring k, and e's round ring is its segments back to back.
 *
 * Work split.  The plan (one workgroup) counts all (id, ring) segments at once:
 * a thread owns four ids and every ring of each, has all their bin_off loads
 * in flight together, sums id-major / ring-minor in registers and scans the
 * per-thread totals twice (slots, tiles).  The pack grid is sized to the
 * device; a tile is USN_DELIVER_TILE consecutive slots of one receiver's ROUND
 * ring, so all a tile writes stays contiguous and a round of many short rings
 * does not turn into many mostly empty tiles.  A tile may span segments: wave 0
 * reads the receiver's nine segment offsets (a lane each), and for every
 * segment the tile intersects cuts that ring's three lists at the segment-local
 * position (lists_cut; in general no multiple of the tile).  The runs of ALL
 * intersected segments then go to LDS side by side -- segment s owns
 * [dst_s, dst_s + cnt_s) of each run array, which holds them because the cnt_s
 * sum to the tile -- and merge in one pass between two barriers, however many
 * segments there are; the merge leaves each slot's ring in an LDS byte.  A tile
 * none of whose segments has a second run after its cut (nearly all tiles of a
 * round of large rings) skips the run arrays, the merge and its barrier: the
 * one run is the order.
 *
 * Rings differ in layout, n, source and n_ep.  The per-ring fields are arrays
 * of eight in the kernel argument; each workgroup of the pack grid copies them
 * to LDS once (static indices: scalar loads), and a lane's frame address comes
 * from an LDS read by the slot's ring byte, never from a divergent index into
 * the argument.  It is formed once per slot, beside the length (the pass that
 * writes src[] / lens[]), and kept in LDS: the gather reads a length and an
 * address per frame and nothing of the ring.  The pointers read back from LDS
 * are used as global ones (the gather stays on global loads, not flat ones).
 *
 * Copy: the fixed-slot gather of usn_deliver.hip over the tile's slots.
 */
#include "usn_deliver_common.h"

namespace usn {
namespace {

using namespace dv;
constexpr uint32_t UNR = 4;                  // frames a lane group has in flight
constexpr uint32_t RM = USN_ROUND_MAX;
static_assert(RM == 8 && RM + 1 <= 64, "a receiver's segment offsets: one lane each, 8e + k");

__global__ __launch_bounds__(PLAN_T) void rdeliver_plan_kernel(RoundDeliverArgs a) {
  __shared__ unsigned long long wsum[PLAN_T / 64];
  __shared__ uint32_t s_recv;
  const uint32_t tid = threadIdx.x, e0 = tid * 4;
  if (tid == 0) s_recv = 0;
  /* per ring: n_ep and for_nic(src) (uniform), then every bin_off entry this
   * thread needs -- ids e0 .. e0 + 4 clamped to n_ep, and the NIC / FLOOD
   * bins' three -- all issued before the first is used, with no branch
   * between them */
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
  uint32_t own[RM][5], tail[RM][3];
#pragma unroll
  for (uint32_t k = 0; k < RM; ++k) {
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) own[k][j] = a.bin_off[k][e0 + j < n_ep[k] ? e0 + j : n_ep[k]];
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) tail[k][j] = a.bin_off[k][n_ep[k] + j];
  }
  /* recv_lists' rule and clamps, per ring: positions clamped to n, hi >= lo;
   * an id at or above n_ep has own[j] == own[j + 1] (both bin_off[n_ep]) */
  uint32_t cnt[4][RM];
  unsigned long long c = 0, tl = 0;
  uint32_t recv = 0;
#pragma unroll
  for (uint32_t k = 0; k < RM; ++k) {
    const uint32_t n = a.n[k];
    uint32_t o[5], q[3];
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) o[j] = own[k][j] < n ? own[k][j] : n;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) q[j] = tail[k][j] < n ? tail[k][j] : n;
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
  uint32_t tlj[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {   // id-major, ring-minor
    uint32_t lo = 0, hi = 0;   // the 64-bit sum by hand: no count widened to a register pair
#pragma unroll
    for (uint32_t k = 0; k < RM; ++k) {
      lo += cnt[j][k];
      hi += lo < cnt[j][k];
    }
    const unsigned long long ct = (unsigned long long)hi << 32 | lo;   // < 2^35
    tlj[j] = (uint32_t)((ct + P - 1) / P);
    c += ct;
    tl += tlj[j];
    recv += ct != 0;
  }
  unsigned long long need = 0, tiles = 0;
  const unsigned long long off = plan_scan(c, wsum, &need);
  const unsigned long long toff = plan_scan(tl, wsum, &tiles);
  if (recv) atomicAdd(&s_recv, recv);
  const bool overflow = need > (unsigned long long)a.cap;
  /* 32 bits from here: a saturating sum is the 64-bit sum saturated, and the
   * tile prefix is only used (and then fits) when need <= cap < 2^32 */
  uint32_t o = sat32(off), tp = (uint32_t)toff;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    a.ep_off[e0 + j] = o;
    a.tile_pfx[e0 + j] = overflow ? 0u : tp;   // on overflow the pack grid gets no tile
    tp += tlj[j];
    uint32_t so[RM];
#pragma unroll
    for (uint32_t k = 0; k < RM; ++k) {
      so[k] = o;
      o = o + cnt[j][k] < o ? 0xFFFFFFFFu : o + cnt[j][k];
    }
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.seg_off + (size_t)(e0 + j) * RM);   // 32-byte aligned
    dst[0] = u32x4{so[0], so[1], so[2], so[3]};
    dst[1] = u32x4{so[4], so[5], so[6], so[7]};
  }
  if (tid == PLAN_T - 1) a.seg_off[(size_t)USN_DT_IDS * RM] = o;   // == need, saturated
  __syncthreads();
  if (tid == 0) {
    a.hdr->need = sat32(need);
    a.hdr->cap = a.cap;
    a.hdr->flags = overflow ? USN_DV_OVERFLOW : 0u;
    a.hdr->n_recv = s_recv;
  }
}

__global__ __launch_bounds__(PACK_T) void rdeliver_pack_kernel(RoundDeliverArgs a) {
  __shared__ uint32_t s_run[3][P];
  __shared__ uint32_t s_src[P];
  __shared__ uint16_t s_len[P];
  __shared__ uint8_t s_rb[P];               // the ring of the tile's slot
  __shared__ uint64_t s_addr[P];            // the address of its frame
  __shared__ uint32_t s_seg[RM][S_WORDS];
  __shared__ uint32_t s_h[4];               // m, out0, intersected segments, none of them merges
  /* the ring table */
  __shared__ const uint8_t *t_frames[RM];
  __shared__ uint64_t t_stride[RM];
  __shared__ const uint64_t *t_offsets[RM];
  __shared__ const uint16_t *t_lens[RM];
  __shared__ const uint32_t *t_index[RM];
  __shared__ const uint32_t *t_bin_off[RM];
  __shared__ uint32_t t_n[RM], t_src[RM], t_n_ep[RM], t_nic[RM];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // stream order makes the plan's header, prefix and segment offsets visible
  if (a.hdr->flags & USN_DV_OVERFLOW) return;
  const uint32_t ntile = a.tile_pfx[USN_DT_IDS - 1];
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
      const uint32_t k0 = (t - a.tile_pfx[e]) * P;   // in the round ring; < its length
      const uint32_t so = a.seg_off[(size_t)e * RM + (lane < RM ? lane : RM)];
      const uint32_t base = __builtin_amdgcn_readlane(so, 0);   // readlane: the tile's bounds stay scalar
      const uint32_t rel = so - base;                // lane k: where segment k starts in the ring
      const uint32_t total = __builtin_amdgcn_readlane(rel, RM);
      const uint32_t m = total - k0 < P ? total - k0 : P;
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
        const uint32_t ltot = len[0] + len[1] + len[2];   // == s1 - s0 (the plan counted the same lists)
        const uint32_t p = b0 - s0 < ltot ? b0 - s0 : ltot;
        const uint32_t cnt = b1 - b0 < ltot - p ? b1 - b0 : ltot - p;
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
        s_h[0] = m;
        s_h[1] = base + k0;
        s_h[2] = ns;
        s_h[3] = plain;
      }
    }
    __syncthreads();
    const uint32_t m = s_h[0], out0 = s_h[1], ns = s_h[2];
    const bool plain = s_h[3] != 0;
    /* every segment's runs, side by side: segment s owns [dst, dst + cnt) of each run array.
     * Where no segment has a second run (nearly every tile of a round of large
     * rings) the one run is the order: straight to s_src, no merge, no barrier */
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
      /* an entry's slot: its place in its run plus its rank in the segment's other two */
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
      if (out0 + i < a.cap) {   // always (need <= cap here)
        a.out_src[out0 + i] = fi;
        a.out_lens[out0 + i] = ln;
      }
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
          if (f < m && out0 + f < a.cap) {
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
              uint8_t *dp = a.out_frames + (uint64_t)(out0 + f0 + u * ngroups) * a.slot + b;
              *reinterpret_cast<u32x4 *>(dp) = v[u];
            }
        }
      }
    }
    __syncthreads();   // the next tile reuses the LDS
  }
}

}  // namespace

hipError_t launch_deliver_round(const RoundDeliverArgs &a, uint32_t pack_grid, hipStream_t stream) {
  hipLaunchKernelGGL(rdeliver_plan_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rdeliver_pack_kernel, dim3(pack_grid), dim3(PACK_T), 0, stream, a);
  return hipGetLastError();
}

}  // namespace usn
