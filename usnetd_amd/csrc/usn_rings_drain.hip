/*
 * usn_rings_drain.hip -- the consumer of a usn_ringset: up to budget[e] of the
 * oldest queued frames of every endpoint ring gathered byte-compact into one
 * region, and the heads moved (usn_rings_drain; gfx950).
 *
 * usn_deliver_rings.hip appends to the rings and moves the tails; nothing on
 * the device moved a head.  Here ring e gives its positions head[e], head[e] +
 * 1, ... (take[e] of them) to output slots [ep_off[e], ep_off[e + 1]), ids
 * ascending, and the frames lie back to back in usn_deliver_packed's layout:
 * each on a 16-byte boundary, zero-padded to it, so ONE copy of [0,
 * need_bytes) carries the whole round to the host.
 *
 * Work split, four launches whatever the ring count is; nothing here waits on
 * another workgroup.
 *
 *   plan  (one workgroup, four ids per thread) ring_off, head, tail and budget
 *         as 16-byte loads, all in flight before the first is used.  avail and
 *         want stay in registers; one scan over want gives the slot prefix,
 *         and the capacity handed out in id order needs nothing else: the
 *         slots before id e are min(cap, sum of want below e), which is also
 *         ep_off[e].  A second scan over ceil(take / P) gives the tile prefix.
 *         from, take, left, ep_off, the tile prefix and the next heads leave as
 *         16-byte stores.
 *   sum   (device-sized grid) a tile is USN_DELIVER_TILE consecutive positions
 *         of one id's selected run; a run never exceeds its ring, so the tile's
 *         ring slots are at most two contiguous spans.  The tile's lens are
 *         read coalesced and ceil16(min(len, slot)) / 16 reduced into
 *         tile_b16[t].  No frame byte moves.
 *   scan  (one workgroup) the packed scan of tile_b16 (blocks of PLAN_T tiles
 *         with a carry, the next block's load in flight): tile_base, ep_boff,
 *         need_bytes, the byte-overflow decision -- and the COMMIT: when the
 *         call fits, head[] = the next heads, 16 bytes per thread.  The heads
 *         move here, before the copy launch has read the slots they release,
 *         only because the producers (usn_deliver_rings, usn_ringset_set_head)
 *         must be stream-ordered behind the whole call: no append can start
 *         between this launch and the next.
 *   copy  (the same grid and tiles) every wave finds the tile's receiver for
 *         itself (no barrier); from[e], the ring base and S - 1 are scalars.
 *         The tile's lens / src are read (two slots per thread), the piece
 *         counts scanned in LDS (s_off), off16 / lens / src stored coalesced,
 *         then the gather runs OUTPUT-STATIONARY: lane i takes 16-byte pieces
 *         i, i + 256, ... of the tile's output, four loads in flight before
 *         the first store.  A piece's frame comes from an upper-bound search
 *         in s_off, or a shift / divide when all frames of the tile have the
 *         same piece count; its source address is formed from (from + k0 + f)
 *         & mask where it is used, never stored per slot.  With 64-byte frames
 *         in 64-byte slots both the reads and the writes of a tile are two
 *         contiguous spans.  The piece that straddles the length is masked:
 *         the pad is zero whatever the ring slot held.
 *
 * Every index is clamped: ring_off to total, take to the ring, a length to the
 * slot -- whatever heads, tails, budgets or the rings' lens hold, no access
 * leaves the ring set or the drain.  The ring set's last id never has a ring
 * (usn_ringset_init), so tile_pfx[USN_DT_IDS - 1] is the tile total.
 *
 * Plain C++ vector loads and stores throughout.
 */
#include "usn_deliver_common.h"

namespace usn {
namespace {

using namespace dv;
constexpr uint32_t UNR = 4;                       // pieces a lane has in flight
constexpr uint32_t SCAN_T = PDELIVER_SCAN_BLOCK;  // one tile per thread and pass
static_assert(SCAN_T == PLAN_T, "plan_scan scans PLAN_T values");
static_assert(P == 2 * PACK_T, "the sum and copy kernels hold two slots of a tile per thread");

__device__ __forceinline__ uint32_t pieces_of(uint32_t len) { return (len + 15u) >> 4; }

/* a tile of the selected runs, the same in every lane of the wave that asks */
struct Tile {
  uint32_t e, k0, m;          // receiver, first position in its run, positions
  uint32_t w0, base, mask;    // ring position of the first, the ring's first slot, S - 1
};

__device__ __forceinline__ Tile tile_of(const DrainArgs &a, uint32_t t, uint32_t lane) {
  Tile x;
  uint32_t e = tile_receiver(a.tile_pfx, t, lane);
  e = e < USN_MAX_ENDPOINTS ? e : USN_MAX_ENDPOINTS - 1u;   // always: the last id has no tile
  const uint32_t k0 = (t - a.tile_pfx[e]) * P;
  const uint32_t take = a.take[e];
  /* the ring: clamped to the set, so a slot below base + S lies inside it */
  uint32_t base = a.ring_off[e], end = a.ring_off[e + 1];
  base = base < a.total ? base : a.total;
  end = end < a.total ? end : a.total;
  const uint32_t S = end > base ? end - base : 0u;
  uint32_t m = take > k0 ? (take - k0 < P ? take - k0 : P) : 0u;
  m = m < S ? m : S;   // always (take <= S): no position without a ring
  x.e = __builtin_amdgcn_readfirstlane(e);
  x.k0 = __builtin_amdgcn_readfirstlane(k0);
  x.m = __builtin_amdgcn_readfirstlane(m);
  x.w0 = __builtin_amdgcn_readfirstlane(a.from[e] + k0);
  x.base = __builtin_amdgcn_readfirstlane(base);
  x.mask = __builtin_amdgcn_readfirstlane(S - 1u);   // S >= 1 wherever m > 0
  return x;
}

__global__ __launch_bounds__(PLAN_T) void drain_plan_kernel(DrainArgs a) {
  __shared__ unsigned long long wsum[PLAN_T / 64];
  __shared__ uint32_t s_recv, s_flags;
  const uint32_t tid = threadIdx.x, e0 = tid * 4;
  if (tid == 0) { s_recv = 0; s_flags = 0; }
  /* everything this thread needs of its four ids, issued before the first use */
  const u32x4 ro4 = *reinterpret_cast<const USN_GLOBAL u32x4 *>(as_global(a.ring_off) + e0);
  const uint32_t ro_end = as_global(a.ring_off)[e0 + 4];
  const u32x4 hd = *reinterpret_cast<const USN_GLOBAL u32x4 *>(as_global(a.head) + e0);
  const u32x4 tl = *reinterpret_cast<const USN_GLOBAL u32x4 *>(as_global(a.tail) + e0);
  const u32x4 bd = *reinterpret_cast<const USN_GLOBAL u32x4 *>(as_global(a.budget) + e0);
  uint32_t ro[5] = {ro4.x, ro4.y, ro4.z, ro4.w, ro_end};
#pragma unroll
  for (uint32_t j = 0; j < 5; ++j) ro[j] = ro[j] < a.total ? ro[j] : a.total;
  const uint32_t head[4] = {hd.x, hd.y, hd.z, hd.w}, tail[4] = {tl.x, tl.y, tl.z, tl.w};
  const uint32_t budget[4] = {bd.x, bd.y, bd.z, bd.w};
  uint32_t S[4], avail[4], want[4];
  unsigned long long want_t = 0;
  uint32_t flags = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    S[j] = ro[j + 1] > ro[j] ? ro[j + 1] - ro[j] : 0u;
    if (e0 + j == USN_DT_IDS - 1u) S[j] = 0;            // the last id never has a ring
    const uint32_t f = tail[j] - head[j];               // free-running
    avail[j] = f <= S[j] ? f : 0u;
    if (S[j] && f > S[j]) flags |= USN_DR_BADCOUNT;     // full for the producer, empty here: say so
    want[j] = avail[j] < budget[j] ? avail[j] : budget[j];
    want_t += want[j];
  }
  /* the slots before id e: min(cap, the wants below e) -- the capacity goes out in id order */
  unsigned long long selected = 0, tiles = 0;
  unsigned long long pw = plan_scan(want_t, wsum, &selected);
  const unsigned long long cap = a.cap;
  uint32_t off[5], take[4], left[4], tlj[4];
  unsigned long long tiles_t = 0;
  uint32_t recv = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    off[j] = (uint32_t)(pw < cap ? pw : cap);
    pw += want[j];
    const uint32_t room = a.cap - off[j];
    take[j] = want[j] < room ? want[j] : room;
    take[j] = take[j] < S[j] ? take[j] : S[j];          // always (want <= avail <= S)
    left[j] = avail[j] - take[j];
    if (left[j]) flags |= USN_DR_MORE;
    tlj[j] = (take[j] + P - 1) / P;                     // take <= S (<= 2^30 as usn_ringset_init lays rings out)
    tiles_t += tlj[j];
    recv += take[j] != 0;
  }
  off[4] = (uint32_t)(pw < cap ? pw : cap);
  const uint32_t tp = (uint32_t)plan_scan(tiles_t, wsum, &tiles);
  if (recv) atomicAdd(&s_recv, recv);
  if (flags) atomicOr(&s_flags, flags);
  *reinterpret_cast<u32x4 *>(a.from + e0) = hd;
  *reinterpret_cast<u32x4 *>(a.take + e0) = u32x4{take[0], take[1], take[2], take[3]};
  *reinterpret_cast<u32x4 *>(a.left + e0) = u32x4{left[0], left[1], left[2], left[3]};
  *reinterpret_cast<u32x4 *>(a.ep_off + e0) = u32x4{off[0], off[1], off[2], off[3]};
  if (tid == PLAN_T - 1) a.ep_off[USN_DT_IDS] = off[4];
  *reinterpret_cast<u32x4 *>(a.tile_pfx + e0) = u32x4{tp, tp + tlj[0], tp + tlj[0] + tlj[1], tp + tlj[0] + tlj[1] + tlj[2]};
  *reinterpret_cast<u32x4 *>(a.next_head + e0) =
      u32x4{head[0] + take[0], head[1] + take[1], head[2] + take[2], head[3] + take[3]};
  __syncthreads();
  if (tid == 0) {   // the sum ORs USN_DV_LONG in; the scan writes need_bytes, taken and the byte overflow
    a.hdr->need_bytes = 0;
    a.hdr->cap_bytes = a.cap_bytes;
    a.hdr->selected = (uint32_t)(selected < cap ? selected : cap);
    a.hdr->taken = 0;
    a.hdr->n_recv = s_recv;
    a.hdr->flags = s_flags;
  }
}

__global__ __launch_bounds__(PACK_T) void drain_sum_kernel(DrainArgs a) {
  __shared__ uint32_t s_w[2][PACK_T / 64];   // by the tile loop's parity: one barrier per tile
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // stream order makes the plan's prefix, from and take visible
  const uint32_t ntile = a.tile_pfx[USN_DT_IDS - 1];
  const USN_GLOBAL uint16_t *lens = as_global(a.lens);
  uint32_t par = 0;
  bool is_long = false;
  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x, par ^= 1u) {
    const Tile x = tile_of(a, t, lane);
    uint32_t q = 0;   // this thread's 16-byte pieces (<= 2 x 4096)
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t i = tid + h * PACK_T;
      if (i < x.m) {
        const uint32_t ln = lens[x.base + ((x.w0 + i) & x.mask)];   // < base + S <= total
        is_long |= ln > a.slot;
        q += pieces_of(ln < a.slot ? ln : a.slot);
      }
    }
    for (uint32_t d = 32; d; d >>= 1) q += __shfl_xor(q, d, 64);
    if (lane == 0) s_w[par][wave] = q;
    __syncthreads();
    if (tid == 0) {
      uint32_t tot = 0;
      for (uint32_t k = 0; k < PACK_T / 64; ++k) tot += s_w[par][k];
      a.tile_b16[t] = tot;
    }
  }
  if (is_long) atomicOr(&a.hdr->flags, USN_DV_LONG);
}

__global__ __launch_bounds__(SCAN_T) void drain_scan_kernel(DrainArgs a) {
  __shared__ unsigned long long wsum[SCAN_T / 64];
  const uint32_t tid = threadIdx.x, e0 = tid * 4;
  const uint32_t ntile = a.tile_pfx[USN_DT_IDS - 1];
  const u32x4 nh = *reinterpret_cast<const USN_GLOBAL u32x4 *>(as_global(a.next_head) + e0);
  unsigned long long carry = 0;
  uint32_t v = tid < ntile ? a.tile_b16[tid] : 0u;
  for (uint32_t t0 = 0; t0 < ntile; t0 += SCAN_T) {
    // the next block's load is in flight over this block's scan (t0 + SCAN_T cannot wrap: ntile < 2^24)
    const uint32_t tn = t0 + SCAN_T + tid;
    const uint32_t vn = tn < ntile ? a.tile_b16[tn] : 0u;
    unsigned long long tot;
    const unsigned long long ex = plan_scan(v, wsum, &tot);
    if (t0 + tid < ntile) a.tile_base[t0 + tid] = carry + ex;
    carry += tot;
    v = vn;
  }
  __syncthreads();   // tile_base is read below by other threads of this workgroup
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t tp = a.tile_pfx[e0 + j];   // e's first tile, or the next receiver's; ntile past the last
    a.ep_boff[e0 + j] = 16ull * (tp < ntile ? a.tile_base[tp] : carry);
  }
  const bool fits = 16ull * carry <= a.cap_bytes;
  /* the commit: the consumed positions are released; the copy launch behind
   * this one still reads them, and no producer runs before it has (stream order) */
  if (fits) *reinterpret_cast<u32x4 *>(a.head + e0) = nh;
  if (tid == 0) {
    a.ep_boff[USN_DT_IDS] = 16ull * carry;
    a.hdr->need_bytes = 16ull * carry;
    if (fits) a.hdr->taken = a.hdr->selected;
    else a.hdr->flags |= USN_DV_OVERFLOW_BYTES;   // no other writer now
  }
}

__global__ __launch_bounds__(PACK_T) void drain_copy_kernel(DrainArgs a) {
  __shared__ uint32_t s_off[P + 1];   // pieces before frame i of the tile; [m .. P] = the tile's total
  __shared__ uint16_t s_len[P];       // min(len, slot)
  __shared__ uint32_t s_w[2][PACK_T / 64];
  __shared__ uint32_t s_q0, s_mixed;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // stream order makes the plan's and the scan's header, prefix and bases visible
  const bool copy = !(a.hdr->flags & USN_DV_OVERFLOW_BYTES);
  const uint32_t ntile = a.tile_pfx[USN_DT_IDS - 1];
  const uint64_t cap16 = a.cap_bytes >> 4;
  const USN_GLOBAL uint16_t *lens = as_global(a.lens);
  const USN_GLOBAL uint32_t *src = as_global(a.src);
  const USN_GLOBAL uint8_t *frames = as_global(a.frames);

  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    /* every wave looks the tile up for itself (cached loads): no LDS and no barrier for it */
    const Tile x = tile_of(a, t, lane);
    const uint32_t out0 = a.ep_off[x.e] + x.k0;
    const uint64_t tbase = a.tile_base[t];
    if (tid == 0) s_mixed = 0;
    uint32_t q[2], inc[2];
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {   // positions tid and tid + PACK_T of the tile
      const uint32_t i = tid + h * PACK_T;
      uint32_t cl = 0;
      if (i < x.m && out0 + i < a.cap) {   // the second: always (ep_off[e] + take <= cap)
        const uint32_t rq = x.base + ((x.w0 + i) & x.mask);   // two contiguous spans over the tile
        const uint32_t ln = lens[rq];
        a.out_lens[out0 + i] = (uint16_t)ln;   // the true length
        a.out_src[out0 + i] = src[rq];
        cl = ln < a.slot ? ln : a.slot;
      }
      s_len[i] = (uint16_t)cl;
      q[h] = pieces_of(cl);
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
    uint32_t before = 0;
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t i = tid + h * PACK_T;
      uint32_t wb = before;
      for (uint32_t k = 0; k < PACK_T / 64; ++k) {
        const uint32_t sw = s_w[h][k];
        if (k < wave) wb += sw;
        before += sw;
      }
      const uint32_t ex = wb + inc[h] - q[h];
      s_off[i] = ex;
      if (i == P - 1) s_off[P] = ex + q[h];
      if (i < x.m) {
        if (q[h] != q0) s_mixed = 1;
        if (out0 + i < a.cap) {
          const uint64_t o = tbase + ex;
          a.out_off16[out0 + i] = o > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)o;
        }
      }
    }
    __syncthreads();
    if (copy) {
      const uint32_t total = s_off[P];
      const bool mixed = s_mixed != 0;
      const int shift = (q0 & (q0 - 1u)) == 0 ? __ffs((int)q0) - 1 : -1;   // q0 >= 1 when total > 0 and not mixed
      for (uint32_t p0 = tid; p0 < total; p0 += PACK_T * UNR) {
        u32x4 v[UNR];
        int nb[UNR];   // bytes of the frame from the piece's start; 0: no piece
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u) {
          const uint32_t p = p0 + u * PACK_T;
          nb[u] = 0;
          if (p < total) {
            uint32_t f, k;
            if (mixed) {
              /* the last frame whose first piece is <= p: frames without a
               * piece and the positions past m share their successor's s_off,
               * so the answer is below m and holds piece p */
              f = 0;
#pragma unroll
              for (uint32_t step = P / 2; step; step >>= 1)
                if (s_off[f + step] <= p) f += step;
              k = p - s_off[f];
            } else {
              f = shift >= 0 ? p >> shift : p / q0;
              k = p - f * q0;
            }
            nb[u] = (int)s_len[f] - (int)(k * 16u);   // >= 1
            /* the ring slot of position f, from the tile's scalars; piece k lies inside the slot:
             * 16 k < ceil16(min(len, slot)) <= slot */
            const uint64_t rq = x.base + ((x.w0 + f) & x.mask);
            v[u] = *reinterpret_cast<const USN_GLOBAL u32x4 *>(frames + rq * a.slot + (uint64_t)k * 16u);
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u)
          if (nb[u] > 0) {
            if (nb[u] < 16) {   // mask_piece, on the global load's vector type
              v[u].x &= keep_mask(nb[u]);
              v[u].y &= keep_mask(nb[u] - 4);
              v[u].z &= keep_mask(nb[u] - 8);
              v[u].w &= keep_mask(nb[u] - 12);
            }
            const uint64_t gp = tbase + p0 + u * PACK_T;
            if (gp < cap16)   // always (need_bytes <= cap_bytes here)
              *reinterpret_cast<u32x4 *>(a.out_frames + gp * 16u) = v[u];
          }
      }
    }
    __syncthreads();   // the next tile reuses the LDS
  }
}

}  // namespace

hipError_t launch_rings_drain(const DrainArgs &a, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(drain_plan_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(drain_sum_kernel, dim3(grid), dim3(PACK_T), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(drain_scan_kernel, dim3(1), dim3(SCAN_T), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(drain_copy_kernel, dim3(grid), dim3(PACK_T), 0, stream, a);
  return hipGetLastError();
}

}  // namespace usn
