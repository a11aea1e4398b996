/*
 * usn_brings_drain.hip -- the consumer of a usn_bringset: up to budget[e] of the
 * oldest queued frames of every byte-compact endpoint ring gathered into one
 * region, and the heads moved (usn_brings_drain; gfx950).
 *
 * usn_deliver_brings.hip appends to the rings and moves tail / btail; nothing
 * on the device moved a head.  The queued bytes of a byte ring are compact
 * already: frames [h, h + take) of ring e are the units pos16[h] .. pos16[h +
 * take] of its unit ring (btail where the take empties the ring), at most two
 * contiguous spans.  So the byte volume of every ring follows from two pos16
 * reads in the plan, and the frame bytes move as a straight unit-for-unit copy
 * that is split by UNITS, not by frames: no length sum, no tile scan, no LDS
 * prefix and no per-piece frame search (usn_rings_drain.hip needs all four).
 *
 * Work split, three launches whatever the ring count is; nothing here waits on
 * another workgroup.
 *
 *   plan   (one workgroup, four ids per thread) desc_off, unit_off, head, tail,
 *          btail and budget as 16-byte loads, all in flight before the first is
 *          used; then one dependent load per id, pos16 at the head descriptor
 *          (p0).  avail and want stay in registers; one scan over want gives
 *          the slot prefix and take (usn_rings_drain's rule).  One more
 *          dependent load per id with 0 < take < avail gives p1; nu = p1 - p0.
 *          A 64-bit scan over nu gives ep_boff, need_bytes and the overflow
 *          decision, and ONE more scan gives both tile prefixes: descriptor
 *          tiles ceil(take / P) in the low and unit tiles ceil(nu / UT) in the
 *          high word of the scanned value (neither total reaches 2^32, so no
 *          carry crosses).  The header is complete here except for `taken` and
 *          the USN_DR_BADDESC the copy launch may OR in.
 *   copy   (device-sized grid) descriptor tiles first, then unit tiles, in one
 *          loop.  A descriptor tile is P positions of one id's selected run, two
 *          per thread: lens / src / pos16 of its at most two contiguous
 *          descriptor spans are read and lens / src / off16 stored coalesced.
 *          The chain check needs the NEXT position's pos16: it comes from a
 *          second coalesced read of pos16 shifted by one (the same cache lines;
 *          a cross-lane shuffle would need LDS or a branch at every wave's and
 *          half-tile's last lane), p1 behind the run's last frame.  A unit tile
 *          is UT units of one id's run: lane i moves units i, i + 256, ... as
 *          16-byte loads and stores, four loads in flight before the first
 *          store.  No LDS, no barrier, no masking: the ring holds the pad.
 *   commit (one workgroup) unless the header says byte overflow or a broken
 *          chain, head[] = from + take as 16-byte stores and taken = selected.
 *          The heads move in the call's LAST launch, after every unit they
 *          release has been read.
 *
 * Every index is clamped: desc_off / unit_off to the totals, take to D, nu to
 * B, a descriptor by & (D - 1), a unit by & (B - 1), output positions to cap /
 * cap_bytes -- whatever the counters, lens or pos16 hold, no access leaves the
 * set or the drain.  The set's last id never has a ring (usn_bringset_init), so
 * both prefixes' entry USN_DT_IDS - 1 is that kind's tile total.
 *
 * Plain C++ vector loads and stores throughout.
 */
#include "usn_deliver_common.h"

namespace usn {
namespace {

using namespace dv;
constexpr uint32_t UT = USN_BDRAIN_UTILE;
constexpr uint32_t UNR = 4;   // units a lane has in flight
static_assert(P == 2 * PACK_T, "a descriptor tile holds two positions per thread");
static_assert((UT & (UT - 1)) == 0 && UT % (PACK_T * UNR) == 0, "a unit tile is whole passes of the workgroup");

__device__ __forceinline__ uint32_t units_of(uint32_t len) {   // usn_deliver_brings' u_j
  const uint32_t u = (len + 15u) >> 4;
  return u ? u : 1u;
}

__device__ __forceinline__ u32x4 ld4(const uint32_t *p, uint32_t i) {
  return *reinterpret_cast<const USN_GLOBAL u32x4 *>(as_global(p) + i);
}

/* ring e's [first, first + size) of an offset array, clamped to the set's total */
__device__ __forceinline__ void ring_span(const uint32_t *off, uint32_t e, uint32_t total, uint32_t &base,
                                          uint32_t &size) {
  uint32_t b = as_global(off)[e], n = as_global(off)[e + 1];
  b = b < total ? b : total;
  n = n < total ? n : total;
  base = b;
  size = n > b ? n - b : 0u;
}

__global__ __launch_bounds__(PLAN_T) void bdrain_plan_kernel(BDrainArgs a) {
  __shared__ unsigned long long wsum[PLAN_T / 64];
  __shared__ uint32_t s_recv, s_flags;
  const uint32_t tid = threadIdx.x, e0 = tid * 4;
  if (tid == 0) { s_recv = 0; s_flags = 0; }
  /* round one: everything this thread needs of its four ids, issued before the first use */
  const u32x4 do4 = ld4(a.desc_off, e0), uo4 = ld4(a.unit_off, e0);
  const uint32_t do_end = as_global(a.desc_off)[e0 + 4], uo_end = as_global(a.unit_off)[e0 + 4];
  const u32x4 hd = ld4(a.head, e0), tl = ld4(a.tail, e0), bt = ld4(a.btail, e0), bd = ld4(a.budget, e0);
  uint32_t dof[5] = {do4.x, do4.y, do4.z, do4.w, do_end}, uof[5] = {uo4.x, uo4.y, uo4.z, uo4.w, uo_end};
#pragma unroll
  for (uint32_t j = 0; j < 5; ++j) {
    dof[j] = dof[j] < a.total_desc ? dof[j] : a.total_desc;
    uof[j] = uof[j] < a.total_units ? uof[j] : a.total_units;
  }
  const uint32_t head[4] = {hd.x, hd.y, hd.z, hd.w}, tail[4] = {tl.x, tl.y, tl.z, tl.w};
  const uint32_t btail[4] = {bt.x, bt.y, bt.z, bt.w}, budget[4] = {bd.x, bd.y, bd.z, bd.w};
  const USN_GLOBAL uint32_t *pos16 = as_global(a.pos16);
  uint32_t D[4], B[4], f[4], p0[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    D[j] = dof[j + 1] > dof[j] ? dof[j + 1] - dof[j] : 0u;
    B[j] = uof[j + 1] > uof[j] ? uof[j + 1] - uof[j] : 0u;
    if (e0 + j == USN_DT_IDS - 1u) D[j] = B[j] = 0;     // the last id never has a ring
    f[j] = tail[j] - head[j];                            // free-running
    /* the one dependent load: pos16 at the head descriptor (< dof + D <= total_desc) */
    p0[j] = D[j] && f[j] ? pos16[dof[j] + (head[j] & (D[j] - 1u))] : 0u;
  }
  /* every result leaves as soon as it is known (16-byte stores): the 1024 threads have 128 VGPRs
   * each, and nothing here may spill */
  *reinterpret_cast<u32x4 *>(a.from + e0) = hd;
  *reinterpret_cast<u32x4 *>(a.p0 + e0) = u32x4{p0[0], p0[1], p0[2], p0[3]};
  uint32_t avail[4], want[4];
  unsigned long long want_t = 0;
  uint32_t flags = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t used = f[j] ? btail[j] - p0[j] : 0u;
    const bool sound = f[j] <= D[j] && f[j] <= used && used <= B[j];   // a frame costs a unit at least
    avail[j] = sound ? f[j] : 0u;
    if (D[j] && f[j] && !sound) flags |= USN_DR_BADCOUNT;   // full for the producer, empty here: say so
    want[j] = avail[j] < budget[j] ? avail[j] : budget[j];
    want_t += want[j];
  }
  /* the slots before id e: min(cap, the wants below e) -- the capacity goes out in id order */
  unsigned long long selected = 0;
  unsigned long long pw = plan_scan(want_t, wsum, &selected);
  const unsigned long long cap = a.cap;
  uint32_t off[5], take[4], left[4];
  uint32_t recv = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    off[j] = (uint32_t)(pw < cap ? pw : cap);
    pw += want[j];
    const uint32_t room = a.cap - off[j];
    take[j] = want[j] < room ? want[j] : room;
    take[j] = take[j] < D[j] ? take[j] : D[j];          // always (want <= avail <= D)
    left[j] = avail[j] - take[j];
    if (left[j]) flags |= USN_DR_MORE;
    recv += take[j] != 0;
  }
  off[4] = (uint32_t)(pw < cap ? pw : cap);
  *reinterpret_cast<u32x4 *>(a.take + e0) = u32x4{take[0], take[1], take[2], take[3]};
  *reinterpret_cast<u32x4 *>(a.left + e0) = u32x4{left[0], left[1], left[2], left[3]};
  *reinterpret_cast<u32x4 *>(a.ep_off + e0) = u32x4{off[0], off[1], off[2], off[3]};
  if (tid == PLAN_T - 1) a.ep_off[USN_DT_IDS] = off[4];
  /* round two: p1 behind a partial take; a ring taken whole ends at btail (with take == D the
   * descriptor of h + take is the head's own) */
  uint32_t nu[4];
  unsigned long long tls[4];   // descriptor tiles low, unit tiles high
  unsigned long long nu_t = 0, tl_t = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const bool partial = take[j] && left[j];
    const uint32_t p1 = partial ? pos16[dof[j] + ((head[j] + take[j]) & (D[j] - 1u))] : btail[j];
    nu[j] = take[j] ? p1 - p0[j] : 0u;
    /* used, once more: a selected ring has f != 0 */
    if (partial && (nu[j] < take[j] || nu[j] > btail[j] - p0[j])) flags |= USN_DR_BADDESC;
    nu[j] = nu[j] < B[j] ? nu[j] : B[j];                // always on a sound chain (nu <= used <= B)
    nu_t += nu[j];
    /* take <= D, nu <= B and the sums of D and of B are below 2^32, so neither tile total reaches
     * 2^32 / P + USN_DT_IDS: no carry crosses from the low word */
    tls[j] = (unsigned long long)((take[j] + P - 1) / P) | ((unsigned long long)((nu[j] + UT - 1) / UT) << 32);
    tl_t += tls[j];
  }
  unsigned long long need16 = 0, tiles = 0;
  unsigned long long pb = plan_scan(nu_t, wsum, &need16);
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    a.ep_boff[e0 + j] = 16ull * pb;
    pb += nu[j];
  }
  if (tid == PLAN_T - 1) a.ep_boff[USN_DT_IDS] = 16ull * pb;
  const bool overflow = 16ull * need16 > a.cap_bytes;
  if (overflow) flags |= USN_DV_OVERFLOW_BYTES;
  if (recv) atomicAdd(&s_recv, recv);
  if (flags) atomicOr(&s_flags, flags);
  unsigned long long pt = plan_scan(tl_t, wsum, &tiles);
  uint32_t dpf[4], upf[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    dpf[j] = (uint32_t)pt;
    upf[j] = overflow ? 0u : (uint32_t)(pt >> 32);   // on byte overflow the copy grid gets no unit tile at all
    pt += tls[j];
  }
  *reinterpret_cast<u32x4 *>(a.dtile_pfx + e0) = u32x4{dpf[0], dpf[1], dpf[2], dpf[3]};
  *reinterpret_cast<u32x4 *>(a.utile_pfx + e0) = u32x4{upf[0], upf[1], upf[2], upf[3]};
  __syncthreads();
  if (tid == 0) {   // the copy ORs USN_DR_BADDESC in; the commit writes taken
    a.hdr->need_bytes = 16ull * need16;
    a.hdr->cap_bytes = a.cap_bytes;
    a.hdr->selected = (uint32_t)(selected < cap ? selected : cap);
    a.hdr->taken = 0;
    a.hdr->n_recv = s_recv;
    a.hdr->flags = s_flags;
  }
}

__global__ __launch_bounds__(PACK_T) void bdrain_copy_kernel(BDrainArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  // stream order makes the plan's header, prefixes, p0, from, take and offsets visible
  const uint32_t ndt = a.dtile_pfx[USN_DT_IDS - 1];
  const uint32_t nut = a.utile_pfx[USN_DT_IDS - 1];   // 0 on byte overflow: no byte of the region is written
  const uint64_t cap16 = a.cap_bytes >> 4;
  const USN_GLOBAL uint16_t *lens = as_global(a.lens);
  const USN_GLOBAL uint32_t *src = as_global(a.src);
  const USN_GLOBAL uint32_t *pos16 = as_global(a.pos16);
  const USN_GLOBAL u32x4 *units = reinterpret_cast<const USN_GLOBAL u32x4 *>(as_global(a.frames));
  u32x4 *out = reinterpret_cast<u32x4 *>(a.out_frames);
  bool broken = false;

  for (uint32_t t = blockIdx.x; t < ndt + nut; t += gridDim.x) {   // ndt + nut < 2^32 (see the plan)
    /* every wave looks the tile up for itself (cached loads): no LDS and no barrier for it */
    const bool desc = t < ndt;
    const uint32_t tk = desc ? t : t - ndt;
    const uint32_t *pfx = desc ? a.dtile_pfx : a.utile_pfx;
    uint32_t e = tile_receiver(pfx, tk, lane);
    e = e < USN_MAX_ENDPOINTS ? e : USN_MAX_ENDPOINTS - 1u;   // always: the last id has no tile
    e = __builtin_amdgcn_readfirstlane(e);
    const uint64_t b0 = a.ep_boff[e] >> 4;                    // the run's first output unit
    const uint32_t p0 = __builtin_amdgcn_readfirstlane(a.p0[e]);
    uint32_t nu = (uint32_t)((a.ep_boff[e + 1] >> 4) - b0);   // <= B <= 2^28
    if (desc) {
      const uint32_t k0 = __builtin_amdgcn_readfirstlane((tk - pfx[e]) * P);
      uint32_t base, D;
      ring_span(a.desc_off, e, a.total_desc, base, D);
      const uint32_t take = a.take[e];
      uint32_t m = take > k0 ? (take - k0 < P ? take - k0 : P) : 0u;
      m = m < D ? m : D;   // always (take <= D): no position without a ring
      m = __builtin_amdgcn_readfirstlane(m);
      base = __builtin_amdgcn_readfirstlane(base);
      const uint32_t mask = __builtin_amdgcn_readfirstlane(D - 1u);   // D >= 1 wherever m > 0
      const uint32_t w0 = __builtin_amdgcn_readfirstlane(a.from[e] + k0);
      const uint32_t out0 = __builtin_amdgcn_readfirstlane(a.ep_off[e] + k0);
      const uint32_t last = take - k0 - 1u;   // the run's last position, tile-relative
      nu = __builtin_amdgcn_readfirstlane(nu);
#pragma unroll
      for (uint32_t h = 0; h < 2; ++h) {   // positions tid and tid + PACK_T of the tile
        const uint32_t i = tid + h * PACK_T;
        if (i < m && out0 + i < a.cap) {   // the second: always (ep_off[e] + take <= cap)
          const uint32_t q = base + ((w0 + i) & mask);   // two contiguous spans over the tile; < base + D
          const uint32_t ln = lens[q], ps = pos16[q];
          /* the next frame's start: the same lines once more, shifted by one */
          const uint32_t nx = i == last ? p0 + nu : pos16[base + ((w0 + i + 1u) & mask)];
          broken |= nx != ps + units_of(ln);
          const uint32_t rel = ps - p0;
          a.out_lens[out0 + i] = (uint16_t)ln;
          a.out_src[out0 + i] = src[q];
          a.out_off16[out0 + i] = sat32(b0 + (rel < nu ? rel : nu));
        }
      }
    } else {
      const uint32_t k0 = __builtin_amdgcn_readfirstlane((tk - pfx[e]) * UT);
      uint32_t base, B;
      ring_span(a.unit_off, e, a.total_units, base, B);
      uint32_t m = nu > k0 ? (nu - k0 < UT ? nu - k0 : UT) : 0u;
      m = m < B ? m : B;   // always (nu <= B)
      m = __builtin_amdgcn_readfirstlane(m);
      base = __builtin_amdgcn_readfirstlane(base);
      const uint32_t mask = __builtin_amdgcn_readfirstlane(B - 1u);   // B >= 1 wherever m > 0
      const uint32_t r0 = __builtin_amdgcn_readfirstlane(p0 + k0);    // the tile's first unit, free-running
      const uint64_t o0 = b0 + k0;
      for (uint32_t i0 = tid; i0 < m; i0 += PACK_T * UNR) {
        u32x4 v[UNR];
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u) {
          const uint32_t i = i0 + u * PACK_T;
          if (i < m) v[u] = units[base + ((r0 + i) & mask)];   // < base + B <= total_units
        }
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u) {
          const uint32_t i = i0 + u * PACK_T;
          if (i < m && o0 + i < cap16)   // the second: always (need_bytes <= cap_bytes here)
            out[o0 + i] = v[u];
        }
      }
    }
  }
  if (broken) atomicOr(&a.hdr->flags, USN_DR_BADDESC);
}

__global__ __launch_bounds__(PLAN_T) void bdrain_commit_kernel(BDrainArgs a) {
  const uint32_t tid = threadIdx.x, e0 = tid * 4;
  // stream order: every unit tile has read what these heads release
  if (a.hdr->flags & (USN_DV_OVERFLOW_BYTES | USN_DR_BADDESC)) return;
  const u32x4 fr = ld4(a.from, e0), tk = ld4(a.take, e0);
  *reinterpret_cast<u32x4 *>(a.head + e0) = fr + tk;
  if (tid == 0) a.hdr->taken = a.hdr->selected;
}

}  // namespace

hipError_t launch_brings_drain(const BDrainArgs &a, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(bdrain_plan_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bdrain_copy_kernel, dim3(grid), dim3(PACK_T), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(bdrain_commit_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  return hipGetLastError();
}

}  // namespace usn
