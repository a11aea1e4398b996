/*
 * usn_deliver.hip -- the per-endpoint output rings, packed on the device
 * (usn_deliver; gfx950).
 *
 * The reference writes each decided frame into its target's ring
 * (src/endpoint.rs:61-74) and copies ARP / EAPOL frames to every other
 * endpoint (mirror_to_all, :340-363).  Here the batch's lists (usn_result:
 * index grouped by bin, bin_off) are final in HBM; a receiver's ring is the
 * merge, by frame index, of up to three of them -- its own bin, the NIC bin
 * when it is the source's NIC, the FLOOD bin unless it is the source -- and
 * the frames' bytes gathered behind one another in slots of `slot` bytes.
 *
 * Work split.  The plan kernel (one workgroup) counts and scans the 4096
 * endpoint ids and hands the pack grid a prefix of output tiles per receiver.
 * The pack grid is sized to the device, not to the batch; a workgroup takes
 * output tiles t, t + grid, ...  A tile is USN_DELIVER_TILE consecutive slots
 * of ONE receiver, so everything a tile writes is contiguous: src[], lens[]
 * and the slots themselves.  Its input is found without any pass over the
 * lists: wave 0 partitions the receiver's three sorted, disjoint lists at the
 * tile's first merged position k0 (a merge-path cut generalised to three
 * lists: a 64-ary search, one candidate frame index per lane, for the
 * smallest index below which exactly k0 entries lie; the candidate range and
 * each list's search window are first narrowed by what k0 and the lists'
 * lengths already imply, so a receiver with one list, or with a short FLOOD
 * list, pays one or two rounds).  The <= P entries after each cut go to LDS;
 * an entry's output slot is its position in its own run plus its lower-bound
 * rank in the other two runs -- no atomics, no dependence on lane order.
 *
 * Copy.  g = min(64, slot / 16) lanes share a frame, each moving 16-byte
 * pieces with one 128-bit global load and store; a group has the loads of
 * four frames in flight before its first store (the gather is bound by the
 * latency of scattered 64-128-byte reads).  Only pieces that start below the
 * frame's length move; the piece that straddles it is zeroed past it.
 */
#include "usn_deliver_common.h"

namespace usn {
namespace {

using namespace dv;   // the receiver rule, plan, cut and merge shared with usn_deliver_packed.hip
constexpr uint32_t UNR = 4;                  // frames a lane group has in flight

__global__ __launch_bounds__(PLAN_T) void deliver_plan_kernel(DeliverArgs a) { (void)plan_body(a); }

__global__ __launch_bounds__(PACK_T) void deliver_pack_kernel(DeliverArgs a) {
  __shared__ uint32_t s_run[3][P];
  __shared__ uint32_t s_src[P];
  __shared__ uint16_t s_len[P];
  __shared__ uint32_t s_h[H_WORDS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // stream order makes the plan's header and prefix visible
  if (a.hdr->flags & USN_DV_OVERFLOW) return;
  const uint32_t ntile = a.tile_pfx[USN_DT_IDS - 1];
  const uint32_t n_ep = batch_n_ep(a);
  const uint32_t nic = a.eptab[a.src];
  const uint32_t pieces = a.slot >> 4;
  const uint32_t g = pieces < 64u ? pieces : 64u;   // lanes per frame
  const uint32_t fpw = 64u / g;                     // frames per wave and pass
  const uint32_t lgrp = lane / g, sub = lane - lgrp * g;
  const uint32_t ngroups = (PACK_T / 64u) * fpw, gid = wave * fpw + lgrp;

  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    if (wave == 0) tile_cut(a, t, n_ep, nic, lane, s_h);
    __syncthreads();
    const uint32_t m = s_h[H_M], out0 = s_h[H_OUT0];
    tile_merge(a, s_h, s_run, s_src, tid);
    __syncthreads();
    bool is_long = false;
    for (uint32_t i = tid; i < m; i += PACK_T) {
      const uint32_t fi = s_src[i];
      const uint16_t ln = fi < a.n ? a.lens[fi] : (uint16_t)0;
      s_len[i] = ln;
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
        uint64_t so[UNR];   // byte offsets from a.frames (keeps the loads global, not flat)
        uint32_t ln[UNR], maxlen = 0;
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u) {
          const uint32_t f = f0 + u * ngroups;
          ln[u] = 0;
          so[u] = 0;
          if (f < m && out0 + f < a.cap) {
            const uint32_t l = s_len[f];
            ln[u] = l < a.slot ? l : a.slot;
            if (l) {
              const uint32_t fi = s_src[f];
              so[u] = a.stride ? (uint64_t)fi * a.stride : a.offsets[fi];
            }
          }
          maxlen = ln[u] > maxlen ? ln[u] : maxlen;
        }
        for (uint32_t b = sub * 16u; b < maxlen; b += g * 16u) {
          uint4 v[UNR];
#pragma unroll
          for (uint32_t u = 0; u < UNR; ++u)
            if (b < ln[u]) v[u] = *reinterpret_cast<const uint4 *>(a.frames + so[u] + b);
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
              *reinterpret_cast<uint4 *>(dp) = v[u];
            }
        }
      }
    }
    __syncthreads();   // the next tile reuses the LDS
  }
}

}  // namespace

hipError_t launch_deliver(const DeliverArgs &a, uint32_t pack_grid, hipStream_t stream) {
  hipLaunchKernelGGL(deliver_plan_kernel, dim3(1), dim3(PLAN_T), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(deliver_pack_kernel, dim3(pack_grid), dim3(PACK_T), 0, stream, a);
  return hipGetLastError();
}

}  // namespace usn
