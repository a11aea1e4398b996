/*
 * usn_deliver_common.h -- what the delivery modes share (usn_deliver.hip: fixed
 * slots, usn_deliver_packed.hip: byte-compact, usn_deliver_round.hip: a poll
 * round's rings in one): the receiver rule, the plan over the 4096 endpoint
 * ids, a tile's receiver, the three-list cut and the rank merge in LDS.  Device
 * code only; A is DeliverArgs or PackedDeliverArgs (the fields used here have
 * the same names in both) or, for recv_lists, one ring of a round
 * (usn_deliver_rings.hip appends such a round to persistent rings).
 */
#ifndef USN_DELIVER_COMMON_H
#define USN_DELIVER_COMMON_H

#include "usn_kernels.h"

namespace usn {
namespace dv {

constexpr uint32_t P = USN_DELIVER_TILE;
constexpr uint32_t PLAN_T = 1024;            // 4 ids per thread
constexpr uint32_t PACK_T = 256;
static_assert(PLAN_T * 4 == USN_DT_IDS, "the plan scans four ids per thread");
static_assert((P & (P - 1)) == 0 && P % PACK_T == 0, "tile shape");

template <class A>
__device__ __forceinline__ uint32_t batch_n_ep(const A &a) {
  const uint32_t v = a.summary->n_ep;
  return v < USN_MAX_ENDPOINTS ? v : USN_MAX_ENDPOINTS;   // bin_off holds USN_MAX_BINS + 1 entries
}

/* The lists receiver e merges, as [lo, hi) positions of index[]: 0 its own
 * bin, 1 the NIC bin, 2 the FLOOD bin (empty where the rule gives it none).
 * Positions are clamped to n: nothing here trusts bin_off to be consistent. */
template <class A>
__device__ __forceinline__ void recv_lists(const A &a, uint32_t e, uint32_t n_ep,
                                           uint32_t nic, uint32_t lo[3], uint32_t hi[3]) {
  for (int r = 0; r < 3; ++r) lo[r] = hi[r] = 0;
  if (e >= USN_MAX_ENDPOINTS || a.eptab[e] == USN_DT_NONE) return;
  if (e < n_ep) { lo[0] = a.bin_off[e]; hi[0] = a.bin_off[e + 1]; }
  if (e == nic) { lo[1] = a.bin_off[n_ep]; hi[1] = a.bin_off[n_ep + 1]; }
  if (e != a.src) { lo[2] = a.bin_off[n_ep + 1]; hi[2] = a.bin_off[n_ep + 2]; }
  for (int r = 0; r < 3; ++r) {
    lo[r] = lo[r] < a.n ? lo[r] : a.n;
    hi[r] = hi[r] < a.n ? hi[r] : a.n;
    if (hi[r] < lo[r]) hi[r] = lo[r];
  }
}

/* exclusive scan over the workgroup's PLAN_T values; *total = their sum */
__device__ __forceinline__ unsigned long long plan_scan(unsigned long long v, unsigned long long *wsum,
                                                        unsigned long long *total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned long long inc = v;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();   // wsum may still be read from the scan before
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned long long base = 0, tot = 0;
  for (uint32_t k = 0; k < PLAN_T / 64; ++k) {
    const unsigned long long s = wsum[k];
    if (k < w) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

/* The plan, one workgroup of PLAN_T threads: ep_off, tile_pfx and the first
 * four header words (need, cap, flags, n_recv).  Returns need > cap. */
template <class A>
__device__ __forceinline__ bool plan_body(const A &a) {
  __shared__ unsigned long long wsum[PLAN_T / 64];
  __shared__ uint32_t s_recv;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_recv = 0;
  const uint32_t n_ep = batch_n_ep(a);
  const uint32_t nic = a.eptab[a.src];   // for_nic(src); USN_DT_NONE / USN_DT_NONIC match no id
  uint32_t cnt[4];
  unsigned long long c = 0, tl = 0;
  uint32_t recv = 0;
  for (uint32_t j = 0; j < 4; ++j) {
    uint32_t lo[3], hi[3];
    recv_lists(a, tid * 4 + j, n_ep, nic, lo, hi);
    cnt[j] = (hi[0] - lo[0]) + (hi[1] - lo[1]) + (hi[2] - lo[2]);   // disjoint lists: <= n
    c += cnt[j];
    tl += (cnt[j] + P - 1) / P;
    recv += cnt[j] != 0;
  }
  unsigned long long need = 0, tiles = 0;
  unsigned long long off = plan_scan(c, wsum, &need);
  unsigned long long toff = plan_scan(tl, wsum, &tiles);
  if (recv) atomicAdd(&s_recv, recv);
  const bool overflow = need > (unsigned long long)a.cap;
  for (uint32_t j = 0; j < 4; ++j) {
    a.ep_off[tid * 4 + j] = off > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)off;
    // on overflow the pack grid gets no tile at all (its total below is 0)
    a.tile_pfx[tid * 4 + j] = overflow ? 0u : (uint32_t)toff;
    off += cnt[j];
    toff += (cnt[j] + P - 1) / P;
  }
  __syncthreads();
  if (tid == 0) {
    a.hdr->need = need > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)need;
    a.hdr->cap = a.cap;
    a.hdr->flags = overflow ? USN_DV_OVERFLOW : 0u;
    a.hdr->n_recv = s_recv;
  }
  return overflow;
}

/* first position in [lo, hi) of idx whose entry is >= v */
__device__ __forceinline__ uint32_t lbound(const uint32_t *idx, uint32_t lo, uint32_t hi,
                                           unsigned long long v) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((unsigned long long)idx[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t keep_mask(int nb) {   // the low nb bytes of a word
  return nb >= 4 ? 0xFFFFFFFFu : nb <= 0 ? 0u : ((1u << (8 * nb)) - 1u);
}

/* zero the bytes of a 16-byte piece past its first nb (1 <= nb < 16) */
__device__ __forceinline__ void mask_piece(uint4 &v, int nb) {
  v.x &= keep_mask(nb);
  v.y &= keep_mask(nb - 4);
  v.z &= keep_mask(nb - 8);
  v.w &= keep_mask(nb - 12);
}

/* The receiver of tile t < ntile, by one whole wave: the last id whose tile
 * prefix is <= t (the prefix is monotone, tile_pfx[0] = 0 and its last entry =
 * ntile > t).  Two 64-way rounds, one load per lane each, instead of twelve
 * dependent loads of a binary search */
__device__ __forceinline__ uint32_t tile_receiver(const uint32_t *tile_pfx, uint32_t t, uint32_t lane) {
  const uint32_t c1 = __popcll(__ballot(tile_pfx[lane * 64u] <= t));
  const uint32_t ebase = (c1 - 1u) * 64u;
  return ebase + __popcll(__ballot(tile_pfx[ebase + lane] <= t)) - 1u;
}

/* what wave 0 hands the workgroup per tile */
enum { H_M = 0, H_OUT0 = 1, H_CUT = 2, H_RL = 5, H_WORDS = 8 };

/* One whole wave: the cuts x[r] of three sorted, disjoint lists (list r =
 * len[r] entries of index[] from position lo[r], entries below n) at merged
 * position k0 <= len[0] + len[1] + len[2]: x[0] + x[1] + x[2] == k0 and every
 * entry before a cut lies below every entry after one.  k0 need not be a
 * multiple of the tile. */
__device__ __forceinline__ void lists_cut(const uint32_t *index, uint32_t n, const uint32_t lo[3],
                                          const uint32_t len[3], uint32_t k0, uint32_t lane,
                                          uint32_t x[3]) {
  const uint32_t total = len[0] + len[1] + len[2];
  for (int r = 0; r < 3; ++r) x[r] = 0;
  if (k0 > 0 && (len[0] == total || len[1] == total || len[2] == total)) {
    for (int r = 0; r < 3; ++r) x[r] = len[r] ? k0 : 0u;   // one list: nothing to search
  } else if (k0 > 0) {
    /* x[r] lies in [xmin, xmax] whatever the entries are; the k0-th merged
     * entry v* lies above list r's entry xmin - 1 and not above its entry k0 */
    uint32_t xmin[3], xmax[3];
    unsigned long long L = 0, H = n;
    for (int r = 0; r < 3; ++r) {
      const uint32_t others = total - len[r];
      xmin[r] = k0 > others ? k0 - others : 0u;
      xmax[r] = k0 < len[r] ? k0 : len[r];
      if (xmin[r] >= 1) {
        const unsigned long long v = (unsigned long long)index[lo[r] + xmin[r] - 1] + 1;
        L = v > L ? v : L;
      }
      if (k0 < len[r]) {
        const unsigned long long v = index[lo[r] + k0];
        H = v < H ? v : H;
      }
    }
    if (L > H) L = H;   // only inconsistent lists
    /* smallest v in [L, H] with k0 entries below it, 64 candidates a round */
    while (L < H) {
      const unsigned long long span = H - L;
      const unsigned long long cand = L + ((span * lane) >> 6);
      uint32_t f = 0;
      for (int r = 0; r < 3; ++r)
        f += lbound(index, lo[r] + xmin[r], lo[r] + xmax[r], cand) - lo[r];
      const unsigned long long ok = __ballot(f >= k0);
      if (ok == 0) {
        L = L + ((span * 63u) >> 6) + 1;
      } else {
        const uint32_t j = (uint32_t)__ffsll((long long)ok) - 1u;
        H = L + ((span * j) >> 6);
        L = j ? L + ((span * (j - 1u)) >> 6) + 1 : H;
      }
    }
    for (int r = 0; r < 3; ++r)
      x[r] = lbound(index, lo[r] + xmin[r], lo[r] + xmax[r], L) - lo[r];
  }
}

/* Wave 0: tile t's receiver, the cut of its up to three sorted, disjoint lists
 * at the tile's first merged position k0, and what follows the cuts: s_h[H_M]
 * slots from output slot s_h[H_OUT0], run r = s_h[H_RL + r] entries of index[]
 * from position s_h[H_CUT + r]. */
template <class A>
__device__ __forceinline__ void tile_cut(const A &a, uint32_t t, uint32_t n_ep, uint32_t nic,
                                         uint32_t lane, uint32_t *s_h) {
  const uint32_t e = tile_receiver(a.tile_pfx, t, lane);
  uint32_t lo[3], hi[3], len[3], x[3];
  recv_lists(a, e, n_ep, nic, lo, hi);
  for (int r = 0; r < 3; ++r) len[r] = hi[r] - lo[r];
  const uint32_t total = len[0] + len[1] + len[2];
  const uint32_t k0 = (t - a.tile_pfx[e]) * P;   // < total
  lists_cut(a.index, a.n, lo, len, k0, lane, x);
  if (lane == 0) {
    const uint32_t m = total - k0 < P ? total - k0 : P;
    s_h[H_M] = m;
    s_h[H_OUT0] = a.ep_off[e] + k0;
    for (int r = 0; r < 3; ++r) {
      const uint32_t rem = len[r] - (x[r] < len[r] ? x[r] : len[r]);
      s_h[H_CUT + r] = lo[r] + x[r];
      s_h[H_RL + r] = rem < m ? rem : m;
    }
  }
}

/* The whole workgroup (PACK_T threads), after tile_cut and a barrier: the runs
 * go to LDS and merge into s_src[0, m); an entry's slot is its place in its
 * run plus its rank in the others.  The caller's barrier follows. */
template <class A>
__device__ __forceinline__ void tile_merge(const A &a, const uint32_t *s_h, uint32_t (*s_run)[P],
                                           uint32_t *s_src, uint32_t tid) {
  const uint32_t m = s_h[H_M];
  uint32_t rl[3];
  for (int r = 0; r < 3; ++r) {
    rl[r] = s_h[H_RL + r];
    const uint32_t cut = s_h[H_CUT + r];
    for (uint32_t i = tid; i < rl[r]; i += PACK_T) s_run[r][i] = a.index[cut + i];
  }
  __syncthreads();
  for (int r = 0; r < 3; ++r) {
    const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
    for (uint32_t i = tid; i < rl[r]; i += PACK_T) {
      const uint32_t v = s_run[r][i];
      const uint32_t pos = i + lbound(s_run[r1], 0, rl[r1], v) + lbound(s_run[r2], 0, rl[r2], v);
      if (pos < m) s_src[pos] = v;
    }
  }
}

/* ---- what the modes over a poll round's rings share (usn_deliver_round.hip,
 * usn_deliver_rings.hip) */
#define USN_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <class T>
__device__ __forceinline__ const USN_GLOBAL T *as_global(const T *p) { return (const USN_GLOBAL T *)p; }

/* recv_lists' view of one ring */
struct RingLists {
  const uint16_t *eptab;
  const uint32_t *bin_off;
  uint32_t src, n;
};

__device__ __forceinline__ uint32_t sat32(unsigned long long v) {
  return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
}

/* what wave 0 hands the workgroup per intersected segment */
enum { S_RING = 0, S_DST = 1, S_CNT = 2, S_CUT = 3, S_RL = 6, S_WORDS = 9 };

}  // namespace dv
}  // namespace usn

#endif
