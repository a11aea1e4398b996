/*
 * usn_deliver_packed.hip -- the per-endpoint output rings, byte-compact
 * (usn_deliver_packed; gfx950).
 *
 * usn_deliver.hip gives every delivered frame a slot of `slot` bytes; with
 * mixed frame sizes (64 / 576 / 1500 in 2048-byte netmap slots) such a region
 * is mostly holes.  Here the frames of output slot 0, 1, ... lie back to back,
 * each on a 16-byte boundary and zero-padded to it, so a receiver's ring is a
 * byte range [ep_boff[e], ep_boff[e + 1]) and the whole delivery one range
 * [0, need_bytes) in which every byte was written.  Receivers, order, tiles
 * (USN_DELIVER_TILE slots of one receiver), the plan, the cut and the merge
 * are usn_deliver's (usn_deliver_common.h).
 *
 * Where a frame starts depends on the lengths of all frames before it, so the
 * work is split in two around a scan:
 *
 *   merge  (device-sized grid) cut + rank-merge per tile as in usn_deliver;
 *          writes src[] / lens[] and reduces the tile's 16-byte pieces,
 *          sum of ceil16(len) / 16, into tile_b16[t].  No frame byte moves.
 *   scan   (one workgroup) exclusive 64-bit scan of tile_b16 in blocks of
 *          PDELIVER_SCAN_BLOCK tiles with a running carry: tile_base[t],
 *          ep_boff[e] = the base of e's first tile (of the next receiver's
 *          for an id without one), need_bytes, the byte-overflow decision.
 *          A separate launch: nothing here waits on another workgroup.
 *   copy   (device-sized grid, the same tiles) reads the tile's src[] /
 *          lens[] back coalesced, scans the pieces per frame in LDS (s_off),
 *          writes off16[], then gathers OUTPUT-STATIONARY: the tile's output
 *          is s_off[P] consecutive 16-byte pieces and lane i takes pieces i,
 *          i + 256, ...  A wave's store is 1 KiB of consecutive bytes whatever
 *          the length mix, and a 1504-byte frame beside 64-byte ones leaves no
 *          lane idle.  A lane finds its piece's frame by a 9-step upper-bound
 *          search in s_off; a tile whose frames all have the same piece count
 *          (every tile of a 64-byte config) divides instead.  Four loads are in
 *          flight per lane before its first store; the piece that straddles
 *          len is zeroed past it.
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
static_assert(P == 2 * PACK_T, "the copy kernel holds two slots of a tile per thread");

__device__ __forceinline__ uint32_t pieces_of(uint32_t len) { return (len + 15u) >> 4; }

__global__ __launch_bounds__(PLAN_T) void pdeliver_plan_kernel(PackedDeliverArgs a) {
  (void)plan_body(a);
  if (threadIdx.x == 0) {   // the scan overwrites need_bytes unless the slots overflowed
    a.hdr->need_bytes = 0;
    a.hdr->cap_bytes = a.cap_bytes;
  }
}

__global__ __launch_bounds__(PACK_T) void pdeliver_merge_kernel(PackedDeliverArgs a) {
  __shared__ uint32_t s_run[3][P];
  __shared__ uint32_t s_src[P];
  __shared__ uint32_t s_h[H_WORDS];
  __shared__ uint32_t s_w[PACK_T / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // stream order makes the plan's header and prefix visible
  if (a.hdr->flags & USN_DV_OVERFLOW) return;
  const uint32_t ntile = a.tile_pfx[USN_DT_IDS - 1];
  const uint32_t n_ep = batch_n_ep(a);
  const uint32_t nic = a.eptab[a.src];

  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    if (wave == 0) tile_cut(a, t, n_ep, nic, lane, s_h);
    __syncthreads();
    const uint32_t m = s_h[H_M], out0 = s_h[H_OUT0];
    tile_merge(a, s_h, s_run, s_src, tid);
    __syncthreads();
    uint32_t q = 0;   // this thread's 16-byte pieces (<= 2 x 4096)
    for (uint32_t i = tid; i < m; i += PACK_T) {
      const uint32_t fi = s_src[i];
      const uint16_t ln = fi < a.n ? a.lens[fi] : (uint16_t)0;
      if (out0 + i < a.cap) {   // always (need <= cap here)
        a.out_src[out0 + i] = fi;
        a.out_lens[out0 + i] = ln;
        q += pieces_of(ln);     // the copy kernel reads exactly these back
      }
    }
    for (uint32_t d = 32; d; d >>= 1) q += __shfl_xor(q, d, 64);
    if (lane == 0) s_w[wave] = q;
    __syncthreads();
    if (tid == 0) {
      uint32_t tot = 0;
      for (uint32_t k = 0; k < PACK_T / 64; ++k) tot += s_w[k];
      a.tile_b16[t] = tot;
    }
    // the next tile's writes of s_h, s_run, s_src and s_w all lie behind its own barriers
  }
}

__global__ __launch_bounds__(SCAN_T) void pdeliver_scan_kernel(PackedDeliverArgs a) {
  __shared__ unsigned long long wsum[SCAN_T / 64];
  const uint32_t tid = threadIdx.x;
  if (a.hdr->flags & USN_DV_OVERFLOW) return;   // need_bytes stays 0, ep_boff unwritten
  const uint32_t ntile = a.tile_pfx[USN_DT_IDS - 1];
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
    const uint32_t e = tid * 4 + j;
    const uint32_t tp = a.tile_pfx[e];   // e's first tile, or the next receiver's; ntile past the last
    a.ep_boff[e] = 16ull * (tp < ntile ? a.tile_base[tp] : carry);
  }
  if (tid == 0) {
    a.hdr->need_bytes = 16ull * carry;
    if (16ull * carry > a.cap_bytes) a.hdr->flags |= USN_DV_OVERFLOW_BYTES;   // no other writer now
  }
}

__global__ __launch_bounds__(PACK_T) void pdeliver_copy_kernel(PackedDeliverArgs a) {
  __shared__ uint32_t s_off[P + 1];   // pieces before frame i of the tile; [m .. P] = the tile's total
  __shared__ uint64_t s_start[P];     // byte offset of frame i from a.frames
  __shared__ uint16_t s_len[P];
  __shared__ uint32_t s_w[2][PACK_T / 64];
  __shared__ uint32_t s_q0, s_mixed;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // stream order makes the plan's and the scan's header, prefix and bases visible
  const uint32_t flags = a.hdr->flags;
  if (flags & USN_DV_OVERFLOW) return;
  const bool copy = !(flags & USN_DV_OVERFLOW_BYTES);
  const uint32_t ntile = a.tile_pfx[USN_DT_IDS - 1];
  const uint64_t cap16 = a.cap_bytes >> 4;

  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    /* every wave looks the receiver up for itself (two cached loads per lane):
     * no LDS and no barrier for it */
    uint32_t e = tile_receiver(a.tile_pfx, t, lane);
    e = e < USN_MAX_ENDPOINTS ? e : USN_MAX_ENDPOINTS - 1u;   // always: the last id has no tile
    const uint32_t k0 = (t - a.tile_pfx[e]) * P;
    const uint32_t e0 = a.ep_off[e], cnt = a.ep_off[e + 1] - e0;
    const uint32_t out0 = e0 + k0;
    const uint32_t m = cnt > k0 ? (cnt - k0 < P ? cnt - k0 : P) : 0u;
    const uint64_t base = a.tile_base[t];
    if (tid == 0) s_mixed = 0;
    uint32_t q[2], inc[2];
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {   // slots tid and tid + PACK_T of the tile
      const uint32_t i = tid + h * PACK_T;
      uint32_t ln = 0;
      uint64_t st = 0;
      if (i < m && out0 + i < a.cap) {
        ln = a.out_lens[out0 + i];
        const uint32_t fi = a.out_src[out0 + i];
        if (fi >= a.n) ln = 0;   // never: the merge kernel stored length 0 for such an entry
        if (ln) st = a.stride ? (uint64_t)fi * a.stride : a.offsets[fi];
      }
      s_len[i] = (uint16_t)ln;
      s_start[i] = st;
      q[h] = pieces_of(ln);
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
      if (i < m) {
        if (q[h] != q0) s_mixed = 1;
        if (out0 + i < a.cap) {
          const uint64_t o = base + ex;
          a.out_off16[out0 + i] = o > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)o;
        }
      }
    }
    __syncthreads();
    if (copy) {
      const uint32_t total = s_off[P];
      const bool mixed = s_mixed != 0;
      const int shift = (q0 & (q0 - 1u)) == 0 ? __ffs((int)q0) - 1 : -1;   // q0 >= 1 when total > 0
      for (uint32_t p0 = tid; p0 < total; p0 += PACK_T * UNR) {
        uint4 v[UNR];
        int nb[UNR];   // bytes of the frame from the piece's start; 0: no piece
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u) {
          const uint32_t p = p0 + u * PACK_T;
          nb[u] = 0;
          if (p < total) {
            uint32_t f, k;
            if (mixed) {
              /* the last frame whose first piece is <= p: frames without a
               * piece and the slots past m share their successor's s_off, so
               * the answer is below m and holds piece p */
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
            v[u] = *reinterpret_cast<const uint4 *>(a.frames + s_start[f] + (uint64_t)k * 16u);
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u)
          if (nb[u] > 0) {
            if (nb[u] < 16) mask_piece(v[u], nb[u]);
            const uint64_t gp = base + p0 + u * PACK_T;
            if (gp < cap16)   // always (need_bytes <= cap_bytes here)
              *reinterpret_cast<uint4 *>(a.out_frames + gp * 16u) = v[u];
          }
      }
    }
    __syncthreads();   // the next tile reuses the LDS
  }
}

}  // namespace

hipError_t launch_deliver_packed(const PackedDeliverArgs &a, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(pdeliver_plan_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pdeliver_merge_kernel, dim3(grid), dim3(PACK_T), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pdeliver_scan_kernel, dim3(1), dim3(SCAN_T), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pdeliver_copy_kernel, dim3(grid), dim3(PACK_T), 0, stream, a);
  return hipGetLastError();
}

}  // namespace usn
