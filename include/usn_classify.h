/*
 * usn_classify.h -- C ABI of the MI355X-native usnetd match path.
 *
 * This is the drop-in boundary for usnetd's per-frame decision path.  The
 * reference has no FFI; the path is internal Rust and is called once per
 * received frame:
 *
 *   Endpoint::forward (drain loop)       /root/reference/src/endpoint.rs:114-171
 *     -> Endpoint::find_forward          /root/reference/src/endpoint.rs:172-296
 *        -> extract_pkt_info             /root/reference/src/pkt.rs:158-218
 *        -> get_endpoint                 /root/reference/src/endpoint.rs:307-338
 *        -> mirror_to_all (FLOOD)        /root/reference/src/endpoint.rs:340-363
 *
 * Here a drained rx ring is one batch resident in HBM and one call classifies
 * all of it.  The state the reference keeps in `main` and in each `Endpoint`
 * (match_register, innerl2bridge, fragmentation_map, listening, last_pkt,
 * last_pkt_dst, next_dhcp_endpoint) lives in a usn_ctx; the rule-registry
 * operations keep the reference's semantics so a host (Rust over this ABI,
 * see INTEGRATION.md, or the C++ control plane) can drive it directly.
 *
 * Conventions: every function returns int status (0 = ok, negative = error,
 * see USN_E*), never throws, never aborts.  Pointers named dev_* or documented
 * "device" are HIP device pointers on the ctx's device.  Nothing here takes
 * or returns a torch type.
 */
#ifndef USN_CLASSIFY_H
#define USN_CLASSIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: usn_result_release; two consecutive tx rings per usn_classify_multi;
 *    usn_finalize waits for the batch's own launch, not the stream
 * 5: up to eight consecutive tx rings per usn_classify_multi */
#define USN_ABI_VERSION 5
#define USN_WINDOW 64     /* default readable header bytes at every frame start (usn_batch.window) */
#define USN_WINDOW_MAX 80 /* the most extract_pkt_info ever reads: L4 ports of IHL 15 end at byte 78 */
#define USN_TILE 1024     /* frames per tile (one classify workgroup; tile headers) */
#define USN_MAX_ENDPOINTS 4095 /* endpoint ids 0..4094 (0xFFFF = none); netmap pipe ids are 12 bits
                                  (/root/reference/src/devices.rs:36-37) */

/* status codes */
#define USN_OK 0
#define USN_EINVAL (-22)
#define USN_ENOMEM (-12)
#define USN_EEXIST (-17)
#define USN_ENOENT (-2)
#define USN_EPERM (-1)
#define USN_EHIP (-5)        /* HIP runtime error; usn_last_hip_error() */
#define USN_ENODEV (-19)     /* no gfx950 device */
#define USN_ERANGE (-34)
#define USN_EBUSY (-16)      /* a tx batch awaits usn_finalize (shared state not final yet) */
#define USN_ELIST (-74)      /* EBADMSG: the device found the batch's per-bin counts disagreeing with
                                its decisions; index / bin_off of that batch are not valid */

/* ---- decision word (u32), one per frame --------------------------------
 *   [15:0]  endpoint id (0xFFFF = none)            Target::Endpoint/EndpointRef
 *   [19:16] class                                  Option<Target>
 *   [23:20] drop reason (informational, exact)
 *   [31:24] flags (informational)
 * Parity with the reference is defined on bits [23:0]. */
#define USN_CLS_DROP 0u    /* None: endpoint.rs:207, 275, 293 */
#define USN_CLS_EP 1u      /* Target::Endpoint / EndpointRef / Last->endpoint */
#define USN_CLS_NIC 2u     /* Target::Nic (endpoint id = the source's NIC) */
#define USN_CLS_FLOOD 3u   /* mirror_to_all: every endpoint except the source */
#define USN_R_NONE 0u
#define USN_R_PARSE 1u     /* extract_pkt_info -> None */
#define USN_R_LOOPBACK 2u  /* endpoint.rs:205-208 */
#define USN_R_NOMATCH 3u   /* endpoint.rs:274-277 */
#define USN_R_EXCLUDED 4u  /* get_endpoint hit a NIC or the source (endpoint.rs:328-336) */
#define USN_R_FRAGMISS 5u  /* later fragment without a remembered first (pkt.rs:172-176) */
#define USN_R_DHCP_NONE 6u /* DHCP answer, no rule, no next_dhcp (endpoint.rs:269-272) */
#define USN_R_WINDOW 7u    /* device: L4 ports lie beyond usn_batch.window; usn_finalize resolves
                              the frame from the host frame reader (usn_set_frame_reader) */
#define USN_F_CACHE (1u << 24)   /* decision taken from the 1-entry cache (endpoint.rs:186-191) */
#define USN_F_FRAG1 (1u << 25)   /* first fragment: remembered in the fragment map */
#define USN_F_FRAGN (1u << 26)   /* later fragment: resolved through the fragment map */
#define USN_F_DHCP (1u << 27)    /* DHCP steering involved */
#define USN_F_HOST (1u << 28)    /* resolved by the ordered host stage (usn_finalize) */
#define USN_F_LEARN (1u << 29)   /* tx: this frame learned a MAC or an answer rule */
#define USN_DEC_CLASS(d) (((d) >> 16) & 0xFu)
#define USN_DEC_EP(d) ((d) & 0xFFFFu)
#define USN_DEC_REASON(d) (((d) >> 20) & 0xFu)
#define USN_PARITY_MASK 0x00FFFFFFu

/* ---- endpoints (all_devices entries; devices.rs:14-25) ------------------ */
#define USN_EP_NIC 0   /* NicNetmap / NicMacVtap: get_nic().is_some() */
#define USN_EP_HOST 1  /* HostRing / HostTap */
#define USN_EP_PIPE 2  /* UserNetmap */
#define USN_EP_UDS 3   /* UserUnixDomainSocket */

/* ---- rule key: Want (pkt.rs:220-227) ------------------------------------ */
#define USN_WANT_DPORT 1u  /* dst_port is Some */
#define USN_WANT_SRC 2u    /* src_addr is Some */
#define USN_WANT_SPORT 4u  /* src_port is Some */
typedef struct {
  uint32_t dst_addr;   /* IPv4 a.b.c.d as (a<<24)|(b<<16)|(c<<8)|d */
  uint32_t src_addr;
  uint16_t dst_port;
  uint16_t src_port;
  uint8_t protocol;
  uint8_t present;     /* USN_WANT_* bits; absent fields are ignored */
  uint16_t _reserved;
} usn_want;

/* ---- batch of frames (one drained rx ring of one source endpoint) -------- */
typedef struct {
  const uint8_t *frames;   /* device: frame i starts at frames + i*stride or frames + offsets[i];
                              16-byte aligned, `window` readable bytes of frame i at every start */
  uint64_t stride;         /* > 0 selects the fixed-stride layout (netmap-slot like) */
  const uint64_t *offsets; /* device, or NULL when stride > 0 */
  const uint16_t *lens;    /* device: frame lengths (netmap_slot.len) */
  uint64_t n;              /* frames in the batch */
  uint16_t src_endpoint;   /* the endpoint whose ring was drained */
  uint16_t window;         /* bytes of frame i readable at its start, >= USN_WINDOW (0 means
                              USN_WINDOW); with a stride, window <= stride.  A frame whose ports
                              lie past the window (IPv4 with IHL >= 12 at window 64: pkt.rs:177-186
                              reads 14+hl .. 18+hl) is never read past it: the kernel flags it
                              USN_R_WINDOW | USN_F_HOST and usn_finalize resolves it from the host
                              frame reader.  window >= USN_WINDOW_MAX never needs the reader. */
  uint16_t _reserved[2];
} usn_batch;

/* Tile header: one per USN_TILE frames (written by the tile's workgroup only,
 * so no device-wide atomics and no per-batch memset are needed). */
typedef struct {
  uint16_t n_frames;       /* frames in this tile */
  uint16_t _r0;
  uint16_t n_host;         /* frames of this tile listed for the ordered host stage */
  uint16_t bin_nic;        /* = usn_summary.n_ep: the bin of Target::Nic (see usn_result.index) */
  uint16_t class_count[4]; /* frames per decision class (before host fix-ups) */
  uint32_t last_state;     /* internal: 1-entry cache state after this tile */
  uint32_t last_dst;
  uint32_t last_idx;
  uint32_t last_info[4];
  uint32_t _pad;
} usn_tile_hdr;            /* 48 bytes */

/* Batch summary (device), written by workgroup 0 and by usn_finalize. */
typedef struct {
  uint32_t flags;          /* USN_S_* */
  uint32_t first_break;    /* stale mode: first frame that ends the stale prefix */
  uint32_t n_frames;
  uint32_t n_tiles;
  uint32_t cin_state, cin_dst, cin_info[4];   /* carried-in cache as resolved on device */
  uint32_t cout_state, cout_dst, cout_info[4];/* carried-out override (finalize) */
  uint32_t n_ep;           /* endpoint bins of usn_result.index: bins 0..n_ep-1 are endpoint ids,
                              n_ep = NIC, n_ep+1 = FLOOD, n_ep+2 = DROP */
  uint32_t n_bins;         /* n_ep + 3: usn_result.bin_off has n_bins + 1 entries */
  uint32_t host_epoch;     /* internal: the launch tag of the last classify whose tiles listed
                              frames for the ordered host stage */
  uint32_t _pad;
} usn_summary;             /* 80 bytes */
#define USN_S_STALE 1u         /* carried cache entry disagrees with the current table */
#define USN_S_STALE_EXTENDS 2u /* stale prefix may continue past tile 0 */
#define USN_S_COUT 8u          /* cout_* is authoritative (set by finalize) */

/* Result buffers (device), carved by usn_result_bind from one allocation.
 *
 * The per-endpoint output (SURVEY §2 scatter_by_endpoint; the reference
 * writes each frame straight into its target's ring, endpoint.rs:61-74, and
 * copies FLOOD frames to every other endpoint, :340-363): `index` holds the
 * batch's frame indices grouped by bin and in frame order within each bin,
 * bin b's frames at index[bin_off[b] .. bin_off[b+1]).  Bins are the
 * endpoint ids 0..n_ep-1, then NIC (Target::Nic, the source's NIC), FLOOD
 * (mirror_to_all: every endpoint but the source) and DROP; n_ep and n_bins
 * are in the summary.  An endpoint receives its own list merged in frame
 * order with the FLOOD list.  Both are final after usn_classify (stream
 * order), and again after usn_finalize where the host stage patched
 * decisions. */
typedef struct {
  uint32_t *decisions;     /* n decision words */
  uint32_t *index;         /* n: frame indices grouped by bin, stable */
  uint32_t *bin_off;       /* USN_MAX_BINS + 1: bin b = index[bin_off[b] .. bin_off[b+1]) */
  usn_tile_hdr *tiles;     /* ceil(n / USN_TILE) */
  usn_summary *summary;    /* 1 */
  uint32_t *host_list;     /* per tile USN_TILE slots: frames for the ordered host stage */
  void *scratch;           /* device scratch of the per-endpoint scatter (per-tile bin counts
                              and list offsets) */
  uint64_t n;
  uint32_t max_bins;       /* bins the scratch holds (a batch with more endpoints: USN_ERANGE) */
  uint32_t bind_tag;       /* internal: distinct per usn_result_bind call (the scratch's state
                              is re-initialised on the first classify after a bind) */
} usn_result;
#define USN_MAX_BINS (USN_MAX_ENDPOINTS + 3)

/* Per-batch outcome of the ordered host stage. */
typedef struct {
  uint32_t n_host;         /* frames resolved on the host */
  uint32_t n_patched;      /* decisions changed by the host stage */
  uint32_t n_learned;      /* tx: MACs + answer rules learned */
  uint32_t flags;          /* summary flags seen */
  uint32_t class_count[4]; /* final per-class frame counts */
} usn_finalize_info;

/* ---- context --------------------------------------------------------------- */
typedef struct usn_ctx usn_ctx;

int usn_abi_version(void);
const char *usn_strerror(int status);
int usn_last_hip_error(void);

/* Binds to HIP device `hip_device` (must be gfx950).  Replaces the daemon
 * state set up in main() (main.rs:447-449: fragmentation_map, match_register,
 * innerl2bridge).  USN_HOST_ONLY gives a registry-only context for a control
 * plane without a GPU: every device entry point (classify, finalize,
 * plumbing) then returns USN_ENODEV -- there is no CPU classify path. */
#define USN_HOST_ONLY (-1)
int usn_ctx_create(int hip_device, usn_ctx **out);
void usn_ctx_destroy(usn_ctx *ctx);

/* ---- several GPUs behind one registry (replicas only) -------
 * One context, one match_register / bridge / fragment map / per-endpoint
 * state (the reference's single daemon, main.rs:447-449), and one device
 * replica of the rule image and bridge set per entry of hip_devices (the same
 * device may appear twice).  Every registry or bridge change -- AddMatch,
 * RemoveMatch, endpoint removal, usn_table_build / usn_bridge_set, and what a
 * tx batch learned (applied by its usn_finalize, endpoint.rs:194-253) -- bumps
 * the image version; a replica uploads the current version before its next
 * batch (the table-version fence), and while a tx batch awaits usn_finalize
 * every classify on every replica returns USN_EBUSY.  usn_classify /
 * usn_classify_multi and the device plumbing calls act on the selected
 * replica (0 after creation); usn_finalize finds the batch's replica itself.
 * A source whose batches move to another replica carries its decision cache
 * across through the host. */
#define USN_MAX_REPLICAS 16
int usn_ctx_create_group(const int *hip_devices, uint32_t n, usn_ctx **out);
int usn_ctx_replicas(usn_ctx *ctx);
int usn_replica_select(usn_ctx *ctx, uint32_t replica);
int usn_replica_device(usn_ctx *ctx, uint32_t replica);

/* Endpoints::add / EntryChange::Add (main.rs:151-166).  for_nic = -1 iff NIC. */
int usn_endpoint_add(usn_ctx *ctx, uint16_t id, int kind, int32_t for_nic);
/* EntryChange::Remove (main.rs:1058-1069): drops the endpoint and its rules.
 * Cached decisions that name it stay (as in the reference). */
int usn_endpoint_remove(usn_ctx *ctx, uint16_t id);

/* add_listening_match (main.rs:266-298): 1 inserted, 0 key exists ("ER"),
 * USN_EPERM owner is a NIC (the reference panics). Clears the owner's NIC
 * decision cache and records the listening triple.  The device image takes
 * the key in place before the next classify (a few slots, not a rebuild). */
int usn_add_match(usn_ctx *ctx, const usn_want *w, uint16_t owner, int sticky);
/* act_on RemoveMatch (main.rs:608-625): 1 removed, 0 absent, USN_EPERM if
 * requester is not the owner.  Does NOT clear any cache (as the reference). */
int usn_remove_match(usn_ctx *ctx, const usn_want *w, uint16_t requester);
/* QueryUsedPorts / introspection: number of rules, and a copy of them. */
int usn_rule_count(usn_ctx *ctx);
int usn_rules_get(usn_ctx *ctx, usn_want *w, uint16_t *owner, uint8_t *sticky, uint32_t cap);
/* Owner of an exact key, or USN_ENOENT. */
int usn_lookup(usn_ctx *ctx, const usn_want *w);

/* Bulk registry load (SURVEY §8b usn_table_build): replaces match_register
 * (main.rs:867) with `n` rules in one call -- e.g. a daemon restoring its
 * table.  Later duplicates of a key are ignored (HashMap::entry().or_insert).
 * Listening triples are not touched (only AddMatch records them); every NIC
 * decision cache is cleared.  Returns the number of rules in the registry. */
typedef struct {
  uint32_t dst_addr, src_addr;
  uint16_t dst_port, src_port;
  uint8_t protocol;
  uint8_t present;     /* USN_WANT_* bits | USN_RULE_STICKY */
  uint16_t endpoint;   /* owner */
} usn_rule;
#define USN_RULE_STICKY 0x80u
int usn_table_build(usn_ctx *ctx, const usn_rule *rules, uint32_t n);

/* ADD_MACS prefill (main.rs:450-462): appends to the inner L2 bridge. */
int usn_bridge_add(usn_ctx *ctx, const uint8_t mac[6]);
int usn_bridge_count(usn_ctx *ctx);
/* Replace the whole bridge with `n` MACs (SURVEY §8b usn_bridge_set). */
int usn_bridge_set(usn_ctx *ctx, const uint8_t (*macs)[6], uint32_t n);
/* 90 s cleanup: fragmentation_map.clear() (main.rs Cleanup handler). */
int usn_frag_clear(usn_ctx *ctx);

/* ---- the hot path ------------------------------------------------------------ */
/* Bytes of a result for n frames, sized for any endpoint count (USN_MAX_BINS:
 * about 24 bytes of scatter scratch per frame); usn_result_bytes_ep sizes it
 * for endpoint ids < max_endpoints (max id + 1; c5's 1002 endpoints: 6 bytes
 * per frame).  usn_result_bind carves a buffer of `bytes` and sets max_bins
 * from what the scratch holds. */
size_t usn_result_bytes(uint64_t n);
size_t usn_result_bytes_ep(uint64_t n, uint32_t max_endpoints);
int usn_result_bind(void *dev_mem, size_t bytes, uint64_t n, usn_result *out);
/* Drops what the context keeps per result (keyed by its arrays: the replica
 * and bins its last batch ran with, a side-stream lists event, the scan
 * scratch's zeroing tag) before the caller frees or re-binds its memory.  An
 * rx batch classified into it and not finalized is waited for first (its
 * launch's completion event, or the side-stream lists event), so nothing of
 * it still writes the memory when this returns.  A source whose carried
 * decision cache lives in this result's tile headers takes the cache to the
 * host first (it stays valid).  USN_EBUSY while the
 * result belongs to a tx batch not yet finalized.  Bind a result once per
 * allocation and reuse it: results are meant to be long-lived, and a context
 * whose caller never releases them keeps one small record per result. */
int usn_result_release(usn_ctx *ctx, const usn_result *r);

/* Classify one batch on `hip_stream` (hipStream_t; NULL = default stream).
 * Asynchronous: writes decisions, the per-endpoint lists (index, bin_off),
 * tile headers and the summary.
 * Consecutive batches of one source may be enqueued back to back; the 1-entry
 * decision cache is carried on the device from the previous batch's result,
 * which must stay allocated until this call's work has been enqueued.
 * A batch sent by a non-NIC endpoint (tx: find_forward with incoming ==
 * false) learns bridge MACs and answer rules; until its usn_finalize every
 * other call that reads or changes the registry returns USN_EBUSY, except
 * the source's next tx ring(s) on the same stream: at most two tx launches
 * (each one ring, or up to eight rings through usn_classify_multi) are in flight,
 * and their rings are finalized in order (a later one first: USN_EBUSY).
 * A launch ran against the state the launch before it started from; when a
 * usn_finalize of the earlier launch's rings changed that state (it learned,
 * or ran a host tail that left another carried cache or DHCP steering), the
 * later launch's rings are decided again on the host from their first
 * frame. */
int usn_classify(usn_ctx *ctx, const usn_batch *b, usn_result *r, void *hip_stream);
/* Several drained rings of DISTINCT sources (e.g. the rx queues of the NICs
 * polled in one poll() round, main.rs:1029-1046) in one launch: b[k] -> r[k],
 * count <= 8.  Same semantics as `count` usn_classify calls.
 * A sending endpoint's (tx) rings: one ring, or up to eight CONSECUTIVE rings
 * of the same source (count <= 8, distinct results) in one grid, each ring's
 * frames following the ring before's: the same decisions, learning and
 * carried cache as `count` usn_classify calls finalized in turn (ring k sees
 * what the rings before it learned on the device, and is decided again on the
 * host only when ring k - 1's usn_finalize ran a host tail or redid it).
 * Finalize the rings in order.  tx rings of different sources: USN_EINVAL.
 * The launch's frame index must fit 32 bits: the sum over rings k < count - 1
 * of ceil(n_k / USN_TILE) * USN_TILE, plus n of the last ring, must be below
 * 2^32 - 1, else USN_ERANGE. */
int usn_classify_multi(usn_ctx *ctx, const usn_batch *b, usn_result *r, uint32_t count,
                       void *hip_stream);

/* Per-endpoint lists on a side stream (off by default).  With on != 0,
 * usn_classify / usn_classify_multi of NIC rings enqueue the classify kernel
 * on the caller's stream and the scatter that builds index / bin_off on a
 * stream of the library's (one per replica), ordered after it: the caller's
 * stream does not wait for the lists, so the next batch's classify overlaps
 * this batch's scatter.  Decisions, tile headers and the summary stay in the
 * caller's stream order.  The lists are final when usn_finalize returns (it
 * waits for them), or in the order of `hip_stream` after usn_lists_wait.  A
 * result is not overwritten by a later classify before its lists are done.
 * tx batches (learning) always build their lists on the caller's stream. */
int usn_set_lists_async(usn_ctx *ctx, int on);
int usn_lists_wait(usn_ctx *ctx, const usn_result *r, void *hip_stream);

/* Ordered host stage for one classified batch.  Waits for the batch's own
 * launches, not for work queued behind them on the stream (a NIC batch whose
 * lists are built on the side stream: for the stream and its lists); for a
 * tx batch `hip_stream` must be the stream the batch was classified on (else
 * USN_EINVAL).  When the batch needs the host stage, its copies and patches
 * are ordered on `hip_stream` and the call returns after them.  A NIC batch
 * with nothing for the host stage (no stale carried cache, no frame listed)
 * reads only the few words its scatter left in host-mapped memory: about one
 * microsecond of host time.
 * Resolves fragments, DHCP steering, stale cache prefixes and tx learning in
 * frame order and patches decisions and the per-endpoint lists on the device.  Must be called
 * before the next usn_classify of the same source whenever the summary has
 * n_host > 0 or flags != 0; calling it always is allowed.  The batch's
 * index / bin_off are not valid when it returns USN_ELIST (the scatter found
 * a decision naming a bin past the batch's bins, or per-tile counts that
 * disagree with the decisions) or USN_EHIP with usn_last_hip_error() ==
 * hipErrorLaunchTimeOut (702: the device gave up waiting inside the lists'
 * scan, bounded at 200 ms); neither has been observed outside the test hook
 * that forces them.  The batch keeps the bins it was classified with
 * (summary n_bins) when endpoints were added since; only a host-stage
 * decision naming such an endpoint rebuilds its lists with today's bins
 * (summary n_ep / n_bins updated).  USN_ERANGE, before any side effect: the
 * batch needs the host stage and today's bins exceed the result's max_bins
 * (a result sized by usn_result_bytes_ep for fewer endpoints than the context
 * has by then).  This is decided before the host stage runs, so it holds even
 * when no resolved decision would name a new endpoint; the batch cannot be
 * finalized into that result -- classify the ring again into a result sized
 * by usn_result_bytes (any endpoint count never gets USN_ERANGE). */
int usn_finalize(usn_ctx *ctx, const usn_batch *b, usn_result *r, void *hip_stream,
                 usn_finalize_info *info);

/* Host frame reader for frames whose ports lie past usn_batch.window: copies
 * up to `cap` bytes (cap >= USN_WINDOW_MAX) of frame `index` of the batch of
 * `src_endpoint` being finalized into `out`, returns the bytes copied (the
 * frame length when shorter) or a negative value on failure.  Called only
 * from usn_finalize, on the calling thread.  Without a reader, usn_finalize
 * of a batch holding such frames returns USN_EINVAL before any side effect
 * (their decisions stay USN_R_WINDOW drops).  NULL fn unregisters. */
typedef int (*usn_frame_reader)(void *user, uint16_t src_endpoint, uint64_t index, uint8_t *out,
                                uint32_t cap);
int usn_set_frame_reader(usn_ctx *ctx, usn_frame_reader fn, void *user);

/* ---- delivery: each endpoint's output ring, packed on the device -----------
 * The step after the decision (the reference writes a frame into its target's
 * ring, endpoint.rs:61-74, and copies ARP / EAPOL frames to every other
 * endpoint, mirror_to_all, :340-363): for a classified batch of source s whose
 * lists are final, receiver e gets, in ascending frame index, every frame that
 * is class EP with ep == e, class NIC when e == for_nic(s), or class FLOOD
 * when e != s; DROP frames go nowhere.  Receivers are the endpoints registered
 * in the context when usn_deliver is called: an id with a non-empty bin that
 * is no longer registered receives nothing, and a registered id at or above
 * the batch's summary.n_ep can only receive FLOOD.  The result is one
 * contiguous, frame-ordered region of whole frames per endpoint (one D2H copy,
 * a sendmmsg vector or a ring).
 *
 * Sizing: need = sum of the receivers' own bins + n_nic + n_flood x
 * (receivers - 1) slots ((receivers) when the source is not registered).
 * When need > cap the plan sets USN_DV_OVERFLOW and no slot is written;
 * ep_off and hdr->need are still valid, so the caller sizes a retry or falls
 * back to the lists.  A frame longer than `slot` is copied truncated to
 * `slot`; lens[k] holds its true length and USN_DV_LONG is set.
 *
 * In output slot k, bytes [0, len) equal the frame and bytes [len,
 * ceil16(len)) are zero (ceil16: rounded up to a multiple of 16); the rest of
 * the slot is not written.  Every delivered frame must be readable over its
 * first ceil16(len) bytes, not just over usn_batch.window.
 *
 * For a batch that needs the host stage, deliver after usn_finalize: the
 * lists are final only then (see usn_result). */
#define USN_HAS_DELIVER 1
#define USN_DELIVER_TILE 512   /* output slots per pack tile (one workgroup pass) */
#define USN_DV_OVERFLOW 1u     /* need > cap: nothing was packed */
#define USN_DV_LONG 2u         /* a delivered frame's len > slot (copied truncated) */
typedef struct {
  uint32_t need;           /* slots this batch needs (sum over receivers) */
  uint32_t cap;            /* slots the delivery holds */
  uint32_t flags;          /* USN_DV_* */
  uint32_t n_recv;         /* receivers with at least one frame */
} usn_delivery_hdr;
typedef struct {
  uint8_t *frames;         /* cap * slot bytes; output slot k at frames + k*slot */
  uint16_t *lens;          /* cap: length of the frame in slot k */
  uint32_t *src;           /* cap: batch frame index the slot was copied from */
  uint32_t *ep_off;        /* USN_MAX_ENDPOINTS + 1: ring of endpoint e = slots [ep_off[e], ep_off[e+1]) */
  usn_delivery_hdr *hdr;   /* followed by the plan's scratch (the pack grid's tile prefix) */
  uint64_t cap;
  uint32_t slot;           /* bytes per output slot: a multiple of 16 */
  uint32_t _r;
} usn_delivery;
/* Bytes of a delivery of cap_slots slots of `slot` bytes (0 for a slot that is
 * 0 or no multiple of 16, or cap_slots 0 or >= 2^32); usn_delivery_bind carves
 * device (or, for layout checks, host) memory of that size: USN_EINVAL for
 * such a slot or cap, USN_ERANGE when `bytes` is too small. */
size_t usn_delivery_bytes(uint64_t cap_slots, uint32_t slot);
int usn_delivery_bind(void *dev_mem, size_t bytes, uint64_t cap_slots, uint32_t slot, usn_delivery *out);
/* Packs the rings of batch `b` classified into `r` (on r's replica).
 * Asynchronous on `hip_stream`, ordered after the result's lists as
 * usn_lists_wait orders them; reads bin_off, index, summary.n_ep and lens on
 * the device; no host synchronisation and no copy in the steady state.  The
 * receiver table (registered ids and their for_nic) is a small device table
 * per replica, uploaded synchronously before the launch only after the
 * endpoint set changed (the device is drained first, so an earlier delivery
 * still reads the table it was launched with).
 * USN_EINVAL: a null pointer, n >= 2^32 - 1, a result no batch was classified
 * into, slot 0 / no multiple of 16 / smaller than a strided batch's stride;
 * USN_EBUSY: r belongs to a tx batch not yet finalized; USN_ENODEV: a
 * USN_HOST_ONLY context. */
int usn_deliver(usn_ctx *ctx, const usn_batch *b, const usn_result *r, usn_delivery *d,
                void *hip_stream);
/* Synchronises `hip_stream` and copies the header to the host: USN_ERANGE
 * when either flag is set (host_out is filled all the same). */
int usn_deliver_info(usn_ctx *ctx, const usn_delivery *d, void *hip_stream,
                     usn_delivery_hdr *host_out);

/* ---- packed delivery: the same rings, byte-compact --------------------------
 * The receiver rule and the order are usn_deliver's; the output has no slots.
 * The frames of output slot 0, 1, ... of all receivers lie back to back in
 * `frames`: slot k's frame starts at frames + 16 * off16[k] and occupies
 * ceil16(lens[k]) bytes, of which [len, ceil16(len)) are zero.  Endpoint e's
 * frames are bytes [ep_boff[e], ep_boff[e+1]) (ep_boff is monotone over all
 * ids; an id that receives nothing has an empty range).  When the delivery
 * fits, every byte of frames[0, need_bytes) is written, so a copy of that
 * range carries no stale data; nothing is truncated (no USN_DV_LONG).  This
 * is the layout for mixed frame sizes (a pcap or byte stream, a byte ring):
 * the region is need_bytes, not need x the largest slot.
 *
 * Overflow.  need > cap: USN_DV_OVERFLOW; hdr->need and ep_off are valid,
 * need_bytes is 0 and nothing else is written.  need <= cap but need_bytes >
 * cap_bytes: USN_DV_OVERFLOW_BYTES; src, lens, off16, ep_off, ep_boff and
 * need_bytes are valid and complete (off16 saturates at 2^32 - 1, which only
 * a need_bytes of 2^36 or more reaches) and no byte of `frames` is written.
 *
 * Every delivered frame must be readable over its first ceil16(len) bytes,
 * not just over usn_batch.window, as for usn_deliver. */
#define USN_HAS_DELIVER_PACKED 1
#define USN_DV_OVERFLOW_BYTES 4u   /* need_bytes > cap_bytes: no frame byte was written */
typedef struct {
  uint32_t need, cap, flags, n_recv;   /* as usn_delivery_hdr */
  uint64_t need_bytes, cap_bytes;      /* sum of ceil16(len) over delivered slots / the region's size */
} usn_pdelivery_hdr;
typedef struct {
  uint8_t  *frames;    /* cap_bytes; slot k's frame at frames + 16 * off16[k] */
  uint32_t *off16;     /* cap: start of slot k in 16-byte units */
  uint16_t *lens;      /* cap */
  uint32_t *src;       /* cap */
  uint32_t *ep_off;    /* USN_MAX_ENDPOINTS + 1: slots of endpoint e = [ep_off[e], ep_off[e+1]) */
  uint64_t *ep_boff;   /* USN_MAX_ENDPOINTS + 1: bytes of endpoint e = [ep_boff[e], ep_boff[e+1]) */
  usn_pdelivery_hdr *hdr;   /* followed by the kernels' scratch */
  uint64_t cap, cap_bytes;
} usn_pdelivery;
/* Bytes of a packed delivery of cap_slots slots and cap_bytes frame bytes: 0
 * unless cap_slots is in [1, 2^32) and cap_bytes a non-zero multiple of 16 of
 * at most 2^36 - 16 (off16 is 32 bits).  usn_pdelivery_bind carves device (or,
 * for layout checks, host) memory of that size into 256-byte aligned arrays:
 * USN_EINVAL for such arguments, USN_ERANGE when `bytes` is too small.  The
 * scratch behind the header holds the tile prefix and, for the most tiles a
 * delivery of cap_slots can have (cap_slots / USN_DELIVER_TILE +
 * USN_MAX_ENDPOINTS + 1), the tiles' byte totals and bases. */
size_t usn_pdelivery_bytes(uint64_t cap_slots, uint64_t cap_bytes);
int usn_pdelivery_bind(void *dev_mem, size_t bytes, uint64_t cap_slots, uint64_t cap_bytes,
                       usn_pdelivery *out);
/* usn_deliver with the packed output: the same validation (without the slot
 * rules), stream order, receiver table and return codes; no host
 * synchronisation and no copy in the steady state. */
int usn_deliver_packed(usn_ctx *ctx, const usn_batch *b, const usn_result *r, usn_pdelivery *d,
                       void *hip_stream);
/* Synchronises `hip_stream` and copies the header to the host: USN_ERANGE
 * when either overflow flag is set (host_out is filled all the same). */
int usn_deliver_packed_info(usn_ctx *ctx, const usn_pdelivery *d, void *hip_stream,
                            usn_pdelivery_hdr *host_out);

/* ---- round delivery: one ring per endpoint for a whole poll round -----------
 * The reference drains every readable endpoint in one poll round and writes
 * each frame straight into its target's ring, so after a round endpoint e
 * holds ONE ring: source 0's frames for it, then source 1's, and so on.
 * usn_deliver_round packs that ring for up to USN_ROUND_MAX drained rings
 * b[k] classified into r[k], k = 0 .. count - 1 in poll order (the order
 * usn_classify_multi took them; they need not come from one classify call,
 * and sources may repeat: consecutive tx rings of a sender, consecutive
 * drains of a NIC).  Every result must be final.
 *
 * Segment (e, k) is exactly what usn_deliver(b[k], r[k]) gives receiver e:
 * the receiver rule, the order, the slot bytes, the zeroed tail up to
 * ceil16(len), the truncation and USN_DV_LONG.  It occupies slots
 * [seg_off[8e + k], seg_off[8e + k + 1]); rings k >= count are empty.
 * ep_off[e] = seg_off[8e], and endpoint e's round ring [ep_off[e],
 * ep_off[e+1]) is its segments back to back.  src[] holds the frame index
 * inside the slot's own ring; the ring follows from seg_off.  need is the sum
 * over the rings of usn_deliver's need; n_recv counts receivers whose round
 * ring is not empty.  need > cap: USN_DV_OVERFLOW, no slot and no src / lens
 * entry is written; need, ep_off and seg_off stay valid. */
#define USN_HAS_DELIVER_ROUND 1
#define USN_ROUND_MAX 8
typedef struct {            /* usn_delivery's arrays, plus the segments */
  uint8_t *frames;
  uint16_t *lens;
  uint32_t *src;
  uint32_t *ep_off;
  uint32_t *seg_off;        /* USN_ROUND_MAX * (USN_MAX_ENDPOINTS + 1) + 1 */
  usn_delivery_hdr *hdr;    /* followed by the kernels' scratch */
  uint64_t cap;
  uint32_t slot, _r;
} usn_rdelivery;
/* As usn_delivery_bytes / usn_delivery_bind, with room for seg_off. */
size_t usn_rdelivery_bytes(uint64_t cap_slots, uint32_t slot);
int usn_rdelivery_bind(void *dev_mem, size_t bytes, uint64_t cap_slots, uint32_t slot,
                       usn_rdelivery *out);
/* Two launches on `hip_stream` whatever count is, ordered after every
 * result's lists; usn_deliver's validation holds for each ring (the slot
 * rules against each strided ring's stride), the receiver table is uploaded
 * once, and the steady state has no host synchronisation and no copy.
 * USN_EINVAL: count 0 or above USN_ROUND_MAX, what usn_deliver refuses for
 * any ring, results classified on different replicas; USN_EBUSY: an r[k] of a
 * tx batch not yet finalized; USN_ENODEV: a USN_HOST_ONLY context. */
int usn_deliver_round(usn_ctx *ctx, const usn_batch *b, const usn_result *r, uint32_t count,
                      usn_rdelivery *d, void *hip_stream);
/* As usn_deliver_info. */
int usn_deliver_round_info(usn_ctx *ctx, const usn_rdelivery *d, void *hip_stream,
                           usn_delivery_hdr *host_out);

/* ---- ring delivery: a poll round appended to persistent endpoint rings -------
 * The modes above write a fresh, exactly sized region per call.  An endpoint of
 * the reference owns ONE ring of fixed size: a write into a full ring fails
 * and that frame alone is lost (endpoint.rs:75-82).  A ring set is that: one
 * circular ring of `slot`-byte slots per endpoint id in device memory, with
 * free-running 32-bit head / tail counters, and usn_deliver_rings appends a
 * poll round to it.  Nothing is sized per call, nothing overflows globally,
 * and a consumer needs only tail[e].
 *
 * For receiver e with S = ring_off[e+1] - ring_off[e] slots (0 or a power of
 * two): segment (e, k) is offered exactly what usn_deliver_round defines (the
 * receiver rule, the order, registered ids only).  fill = tail[e] - head[e]
 * in 32-bit arithmetic and free = S - min(fill, S): a head "ahead of" the
 * tail, a fill above S and S = 0 all give free = 0.  The first min(offered,
 * free) frames of e's round ring, in round order, are accepted, the rest are
 * dropped (nothing is consumed within a call): seg_acc[8e + k] is segment k's
 * accepted share, acc[e] their sum, drop[e] the rest (saturating), first[e]
 * the tail before the call.  Accepted frame j lands in slot ring_off[e] +
 * ((first[e] + j) & (S - 1)); lens[], src[] and the slot bytes follow
 * usn_deliver (bytes [0, len) the frame, [len, ceil16(len)) zero, truncated
 * at `slot` with USN_DV_LONG, which only an ACCEPTED frame sets).  No other
 * slot is touched, slots between head and tail are never overwritten, and a
 * dropped frame's bytes and list entries are never read.
 *
 * tail[e] becomes first[e] + acc[e] in the call's last launch only, after
 * every slot of the call is written: a reader ordered behind the call (stream
 * or event) sees complete slots below tail.  Calls on one ring set must be
 * stream-ordered with each other and with head updates. */
#define USN_HAS_DELIVER_RINGS 1
#define USN_DV_DROPPED 8u   /* at least one offered frame found its ring full */
typedef struct {
  uint64_t offered;     /* frames the round's rule gives all receivers (usn_deliver_round's need, unsaturated) */
  uint64_t dropped;     /* offered - accepted */
  uint32_t accepted;    /* slots written by this call */
  uint32_t n_recv;      /* receivers with accepted > 0 */
  uint32_t flags;       /* USN_DV_LONG (an ACCEPTED frame longer than slot), USN_DV_DROPPED */
  uint32_t _r;
} usn_ringset_hdr;
typedef struct {
  uint8_t  *frames;     /* total * slot bytes */
  uint16_t *lens;       /* total */
  uint32_t *src;        /* total: frame index inside the slot's own source ring */
  uint32_t *ring_off;   /* USN_MAX_ENDPOINTS + 2: ring of id e = slots [ring_off[e], ring_off[e+1]) */
  uint32_t *head;       /* USN_MAX_ENDPOINTS + 1, free-running, written by the consumer only */
  uint32_t *tail;       /* USN_MAX_ENDPOINTS + 1, free-running, written by the commit launch only */
  uint32_t *first;      /* per id: tail[e] before this call */
  uint32_t *acc;        /* per id: frames accepted by this call */
  uint32_t *drop;       /* per id: frames dropped by this call (saturating) */
  uint32_t *seg_acc;    /* USN_ROUND_MAX * (USN_MAX_ENDPOINTS + 1): accepted frames of segment (e, k) at [8e + k] */
  usn_ringset_hdr *hdr; /* followed by the kernels' scratch (tile prefix, next tails) */
  uint64_t total;
  uint32_t slot, ready; /* ready: set by usn_ringset_init */
} usn_ringset;
/* Bytes of a ring set of total_slots slots of `slot` bytes: 0 unless slot is a
 * non-zero multiple of 16 and total_slots lies in [1, 2^32).  usn_ringset_bind
 * carves device (or, for layout checks, host) memory of that size into
 * 256-byte aligned arrays and clears `ready`: USN_EINVAL for such arguments,
 * USN_ERANGE when `bytes` is too small.  Both only carve memory. */
size_t usn_ringset_bytes(uint64_t total_slots, uint32_t slot);
int usn_ringset_bind(void *dev_mem, size_t bytes, uint64_t total_slots, uint32_t slot, usn_ringset *out);
/* Lays the rings out back to back: ring_slots[e], e < n_ids <=
 * USN_MAX_ENDPOINTS, is 0 or a power of two of at most 2^30, ids from n_ids on
 * get 0, and the sum must not exceed total (else USN_EINVAL).  Uploads
 * ring_off, zeroes head, tail, the per-call arrays and the header, and sets
 * `ready`.  A setup call: it synchronises `hip_stream`. */
int usn_ringset_init(usn_ctx *ctx, usn_ringset *rs, const uint32_t *ring_slots, uint32_t n_ids,
                     void *hip_stream);
/* Copies absolute head counters for ids below n_ids on `hip_stream` and returns
 * when the caller's array may be reused.  `head` is ordinary device memory: a
 * consumer may write it by any other means ordered with the calls. */
int usn_ringset_set_head(usn_ctx *ctx, usn_ringset *rs, const uint32_t *head, uint32_t n_ids,
                         void *hip_stream);
/* usn_deliver_round's arguments, validation (the slot rules against rs->slot),
 * event waits, receiver table and return codes, plus USN_EINVAL for a ring set
 * that is not ready.  Three launches on `hip_stream` whatever count is (plan,
 * pack, commit); no host synchronisation and no copy in the steady state. */
int usn_deliver_rings(usn_ctx *ctx, const usn_batch *b, const usn_result *r, uint32_t count,
                      usn_ringset *rs, void *hip_stream);
/* Synchronises `hip_stream` and copies the header to the host: USN_ERANGE
 * when either flag is set (host_out is filled all the same). */
int usn_deliver_rings_info(usn_ctx *ctx, const usn_ringset *rs, void *hip_stream,
                           usn_ringset_hdr *host_out);

/* ---- ring drain: the endpoint rings' queued frames gathered on the device ----
 * The consumer of a usn_ringset.  One call takes up to budget[e] frames from
 * every ring, oldest first, lays them byte-compact in one region
 * (usn_deliver_packed's layout) so that ONE copy of frames[0, need_bytes)
 * carries the whole round to the host, and advances the heads.
 *
 * Per id e, with S = ring_off[e+1] - ring_off[e], f = tail[e] - head[e] in
 * 32-bit arithmetic and h = head[e] as found: avail = f <= S ? f : 0.  A ring
 * with S > 0 and f > S has corrupt counters: it is not drained and sets
 * USN_DR_BADCOUNT (it would be full for the producer and empty for the
 * consumer for good).  want = min(avail, budget[e]); the slot capacity is
 * handed out in id order, take[e] = min(want[e], cap - min(cap, sum of want
 * below e)); left[e] = avail - take[e], and any left > 0 sets USN_DR_MORE;
 * from[e] = h.  Output slots [ep_off[e], ep_off[e+1]) hold ring positions h,
 * h + 1, ... in that order, ids ascending.  Output slot k, taken from ring
 * slot q = ring_off[e] + ((h + j) & (S - 1)), has lens[k] = rs->lens[q] (the
 * true length) and src[k] = rs->src[q]; with clen = min(lens[k], rs->slot) its
 * bytes lie at frames + 16 * off16[k] and occupy ceil16(clen) bytes: [0, clen)
 * the ring slot's, [clen, ceil16(clen)) zero whatever the slot held.  Frames
 * lie back to back over all ids, ep_boff is monotone as in usn_deliver_packed,
 * and USN_DV_LONG is set when a selected frame has lens > rs->slot.
 *
 * Bytes are all or nothing.  need_bytes = the sum of ceil16(clen) over the
 * selected frames.  need_bytes > cap_bytes: USN_DV_OVERFLOW_BYTES; every
 * metadata array and need_bytes are valid and complete, no byte of `frames` is
 * written and NO HEAD MOVES.  Otherwise every byte of frames[0, need_bytes) is
 * written, nothing past it, and head[e] += take[e].  Ring slots, rs->lens,
 * rs->src and tail are never written.
 *
 * The heads move in the call's third launch, before its last launch has read
 * the slots they release.  That is safe only because usn_rings_drain must be
 * stream-ordered with the appends (usn_deliver_rings) and head updates
 * (usn_ringset_set_head) of the same ring set: no producer runs inside the
 * call.  A producer ordered by anything weaker than the stream (or an event
 * recorded behind the whole call) must not look at head[]. */
#define USN_HAS_RINGS_DRAIN 1
#define USN_DR_MORE 16u       /* a ring keeps queued frames after the call (budget or capacity) */
#define USN_DR_BADCOUNT 32u   /* a ring's tail - head exceeds its size: not drained */
typedef struct {
  uint64_t need_bytes, cap_bytes;   /* sum of ceil16(clen) over the selected frames / the region's size */
  uint32_t selected;    /* sum of take[] */
  uint32_t taken;       /* selected, or 0 on byte overflow (no head moved) */
  uint32_t n_recv;      /* ids with take > 0 */
  uint32_t flags;       /* USN_DV_OVERFLOW_BYTES, USN_DV_LONG, USN_DR_MORE, USN_DR_BADCOUNT */
} usn_drain_hdr;
typedef struct {
  uint8_t  *frames;     /* cap_bytes; output slot k's frame at frames + 16 * off16[k] */
  uint32_t *off16;      /* cap */
  uint16_t *lens;       /* cap: true lengths */
  uint32_t *src;        /* cap */
  uint32_t *ep_off;     /* USN_MAX_ENDPOINTS + 2: slots of id e = [ep_off[e], ep_off[e+1]) */
  uint64_t *ep_boff;    /* USN_MAX_ENDPOINTS + 2: bytes of id e = [ep_boff[e], ep_boff[e+1]) */
  uint32_t *budget;     /* USN_MAX_ENDPOINTS + 1, input: the most frames to take from ring e */
  uint32_t *from;       /* per id: head[e] before this call */
  uint32_t *take;       /* per id: frames selected by this call */
  uint32_t *left;       /* per id: frames still queued behind them */
  usn_drain_hdr *hdr;   /* followed by the kernels' scratch */
  uint64_t cap, cap_bytes;
} usn_drain;
/* usn_pdelivery_bytes / usn_pdelivery_bind's argument rules and 256-byte
 * aligned carving: cap_slots in [1, 2^32), cap_bytes a non-zero multiple of 16
 * of at most 2^36 - 16; 0 / USN_EINVAL for such arguments, USN_ERANGE when
 * `bytes` is too small.  Host memory is accepted for layout checks. */
size_t usn_drain_bytes(uint64_t cap_slots, uint64_t cap_bytes);
int usn_drain_bind(void *dev_mem, size_t bytes, uint64_t cap_slots, uint64_t cap_bytes, usn_drain *out);
/* As usn_ringset_set_head: copies the budgets of ids below n_ids on
 * `hip_stream` (ids from n_ids on get 0) and returns when the caller's array
 * may be reused.  The budgets stay until the next call: a consumer sets them
 * once. */
int usn_drain_set_budget(usn_ctx *ctx, usn_drain *d, const uint32_t *budget, uint32_t n_ids,
                         void *hip_stream);
/* Four launches on `hip_stream` (plan, sum, scan with the commit, copy); no
 * host synchronisation and no copy in the steady state.  USN_EINVAL: a null
 * pointer, a ring set that is not ready, a drain that was not bound;
 * USN_ENODEV: a USN_HOST_ONLY context. */
int usn_rings_drain(usn_ctx *ctx, usn_ringset *rs, usn_drain *d, void *hip_stream);
/* Synchronises `hip_stream` and copies the header to the host: USN_ERANGE when
 * USN_DV_OVERFLOW_BYTES or USN_DR_BADCOUNT is set (host_out is filled all the
 * same).  USN_DR_MORE and USN_DV_LONG alone return 0: they are the normal
 * state of a budgeted consumer. */
int usn_rings_drain_info(usn_ctx *ctx, const usn_drain *d, void *hip_stream, usn_drain_hdr *host_out);

/* ---- byte-ring delivery: persistent endpoint rings, byte-compact -------------
 * usn_deliver_rings' lifetime with usn_deliver_packed's layout.  A byte ring
 * set holds, per endpoint id e, a descriptor ring of D[e] entries (0 or a power
 * of two of at most 2^30) and a byte ring of B[e] 16-byte units (0 or a power
 * of two of at most 2^28; D and B are both zero or both not): descriptors
 * [desc_off[e], desc_off[e+1]) of lens / src / pos16, units [unit_off[e],
 * unit_off[e+1]) of frames.  head / tail count frames and btail counts units,
 * all free-running in 32 bits.  pos16[q] is the free-running unit position of
 * the first unit of the frame in descriptor q.  THERE IS NO BYTE HEAD: a
 * consumer moves head[e] only, and the units ring e holds are 0 when head ==
 * tail, else btail[e] - pos16[desc_off[e] + (head[e] & (D - 1))] in 32-bit
 * arithmetic; the bytes of queued frames [h, h + t) follow from two pos16
 * reads and are at most two contiguous spans.
 *
 * usn_deliver_brings offers receiver e exactly usn_deliver_round's round ring
 * (segments k = 0 .. count - 1, the receiver rule, registered ids only).  Frame
 * j of it has u_j = max(1, ceil16(len_j) / 16) units.  With fill = tail - head,
 * free_d = D - min(fill, D) and free_u = B - min(used, B) (a head ahead of the
 * tail, used > B and D = 0 all give no room), frame j is accepted iff j <
 * free_d and the sum of u_i over i <= j is at most free_u: ONE cut, the
 * accepted frames are a prefix, a frame never overtakes an earlier one, and
 * nothing is consumed within a call.  Accepted frame j gets descriptor
 * desc_off[e] + ((first[e] + j) & (D - 1)) with lens = its true length, src =
 * its index inside its own source ring and pos16 = bfirst[e] + the sum of u_i
 * over i < j; its unit k lies at byte 16 * (unit_off[e] + ((pos16 + k) & (B -
 * 1))), so a frame may straddle the ring's end at any unit boundary.  Bytes
 * [0, len) are the frame and [len, ceil16(len)) zero; nothing is truncated (no
 * USN_DV_LONG).  first / bfirst are tail / btail before the call, acc / drop
 * (saturating) / acc_units the receiver's accepted frames, dropped frames and
 * accepted units, seg_acc[8e + k] segment k's accepted share.
 *
 * No descriptor and no byte between head and tail is written, nothing of
 * frames, lens, src or pos16 outside the accepted frames' descriptors and units
 * is written (staging lives in the scratch behind hdr), and a dropped frame's
 * bytes are never read (its length is: the cut depends on it).  tail[e] +=
 * acc[e] and btail[e] += acc_units[e] happen in the call's last launch only.
 * Calls on one set must be stream-ordered with each other and with head
 * updates.  usn_brings_drain (below) is the device consumer: it gathers frames
 * head .. tail - 1 of every ring through lens / src / pos16 and moves the heads. */
#define USN_HAS_DELIVER_BRINGS 1
typedef struct {
  uint64_t offered;         /* frames the round's rule gives all receivers */
  uint64_t dropped;         /* offered - accepted */
  uint64_t accepted_units;  /* 16-byte units appended by this call */
  uint32_t accepted;        /* frames appended by this call */
  uint32_t n_recv;          /* receivers with accepted > 0 */
  uint32_t flags;           /* USN_DV_DROPPED */
  uint32_t _r;
} usn_bringset_hdr;
typedef struct {
  uint8_t  *frames;     /* total_units * 16 bytes */
  uint16_t *lens;       /* total_desc: true lengths */
  uint32_t *src;        /* total_desc: frame index inside the frame's own source ring */
  uint32_t *pos16;      /* total_desc: free-running unit position of the frame's first unit */
  uint32_t *desc_off;   /* USN_MAX_ENDPOINTS + 2: exclusive prefix of D */
  uint32_t *unit_off;   /* USN_MAX_ENDPOINTS + 2: exclusive prefix of B */
  uint32_t *head;       /* USN_MAX_ENDPOINTS + 1, frames, written by the consumer only */
  uint32_t *tail;       /* USN_MAX_ENDPOINTS + 1, frames, written by the call's last launch only */
  uint32_t *btail;      /* USN_MAX_ENDPOINTS + 1, units, written by the call's last launch only */
  uint32_t *first;      /* per id: tail[e] before this call */
  uint32_t *bfirst;     /* per id: btail[e] before this call */
  uint32_t *acc;        /* per id: frames accepted by this call */
  uint32_t *drop;       /* per id: frames dropped by this call (saturating) */
  uint32_t *acc_units;  /* per id: units accepted by this call */
  uint32_t *seg_acc;    /* USN_ROUND_MAX * (USN_MAX_ENDPOINTS + 1): accepted frames of segment (e, k) at [8e + k] */
  usn_bringset_hdr *hdr;   /* followed by the kernels' scratch (plan, staging, tile sums) */
  uint64_t total_desc, total_units;
  uint32_t ready, _r;   /* ready: set by usn_bringset_init */
} usn_bringset;
/* Bytes of a byte ring set: 0 unless total_desc and total_units both lie in
 * [1, 2^32).  usn_bringset_bind carves device (or, for layout checks, host)
 * memory of that size into 256-byte aligned arrays and clears `ready`:
 * USN_EINVAL for such arguments, USN_ERANGE when `bytes` is too small.  The
 * scratch holds a staging entry per descriptor and the sums of total_desc /
 * USN_DELIVER_TILE + USN_MAX_ENDPOINTS + 2 tiles. */
size_t usn_bringset_bytes(uint64_t total_desc, uint64_t total_units);
int usn_bringset_bind(void *dev_mem, size_t bytes, uint64_t total_desc, uint64_t total_units,
                      usn_bringset *out);
/* Lays both rings of ids below n_ids <= USN_MAX_ENDPOINTS out back to back
 * (ids from n_ids on get none): USN_EINVAL for a size that is no power of two,
 * a D above 2^30 or a B above 2^28, a pair of which only one is zero, or sums
 * above the totals.  Uploads desc_off / unit_off, zeroes the counters, the
 * per-call arrays and the header, and sets `ready`.  A setup call: it
 * synchronises `hip_stream`. */
int usn_bringset_init(usn_ctx *ctx, usn_bringset *rs, const uint32_t *ring_desc,
                      const uint32_t *ring_units, uint32_t n_ids, void *hip_stream);
/* As usn_ringset_set_head. */
int usn_bringset_set_head(usn_ctx *ctx, usn_bringset *rs, const uint32_t *head, uint32_t n_ids,
                          void *hip_stream);
/* usn_deliver_rings' arguments, validation (without the slot rules), event
 * waits, receiver table and return codes, plus USN_EINVAL for a set that is
 * not ready.  Five launches on `hip_stream` whatever count is (plan, merge,
 * scan, copy, commit); no host synchronisation and no copy in the steady
 * state. */
int usn_deliver_brings(usn_ctx *ctx, const usn_batch *b, const usn_result *r, uint32_t count,
                       usn_bringset *rs, void *hip_stream);
/* Synchronises `hip_stream` and copies the header to the host: USN_ERANGE
 * when USN_DV_DROPPED is set (host_out is filled all the same). */
int usn_deliver_brings_info(usn_ctx *ctx, const usn_bringset *rs, void *hip_stream,
                            usn_bringset_hdr *host_out);

/* ---- byte-ring drain: the byte rings' queued frames gathered on the device ---
 * The consumer of a usn_bringset, into the ring drain's region: usn_drain,
 * usn_drain_bytes, usn_drain_bind, usn_drain_set_budget and usn_drain_hdr serve
 * both drains unchanged.  One call takes up to budget[e] frames from every
 * ring, oldest first, lays their units back to back so that ONE copy of
 * frames[0, need_bytes) carries the whole round to the host, and advances the
 * heads.
 *
 * Per id e, with D and B the sizes of its descriptor and unit rings, h =
 * head[e] as found, f = tail[e] - head[e] in 32-bit arithmetic, p0 = pos16 at
 * the head descriptor desc_off[e] + (h & (D - 1)) and used = f ? btail[e] - p0
 * : 0: avail = f when f <= D and f <= used <= B (every frame costs at least one
 * unit, so used >= f on a sound ring), else 0.  A ring with D > 0 and f != 0
 * that fails this has corrupt counters: it is not drained and sets
 * USN_DR_BADCOUNT.  The selection is usn_rings_drain's: want = min(avail,
 * budget[e]), take[e] = min(want[e], cap - min(cap, sum of want below e)),
 * left[e] = avail - take[e] (any left > 0 sets USN_DR_MORE), from[e] = h, and
 * ep_off is the slot prefix, ids ascending.
 *
 * Bytes.  p1 = btail[e] when take == avail, else pos16 at descriptor
 * desc_off[e] + ((h + take) & (D - 1)) (a full ring taken whole has take == D,
 * where that descriptor is the head's own: hence btail).  nu[e] = p1 - p0 in
 * 32-bit arithmetic, 0 when take is 0; ep_boff[e+1] - ep_boff[e] = 16 * nu[e]
 * and need_bytes = 16 * the sum of nu.  Output byte ep_boff[e] + 16 i + b is
 * byte b of unit unit_off[e] + ((p0 + i) & (B - 1)): the ring's units are
 * copied verbatim, pad included (zero where usn_deliver_brings wrote it).  A
 * frame therefore occupies 16 * max(1, ceil16(len) / 16) bytes, which differs
 * from usn_rings_drain's layout only for a zero-length frame: it keeps its one
 * unit.  Nothing is truncated and USN_DV_LONG is never set.
 *
 * Descriptors.  Output slot k = ep_off[e] + j comes from descriptor q =
 * desc_off[e] + ((h + j) & (D - 1)): lens[k] and src[k] are copied from it and
 * off16[k] = ep_boff[e] / 16 + min(pos16[q] - p0, nu[e]).  Inconsistent
 * descriptors are never hidden: for every selected frame the next frame's
 * pos16 (p1 behind the last selected one) must equal its own plus max(1,
 * ceil16(lens) / 16), and a partial take must have take <= nu <= used.  Any
 * violation sets USN_DR_BADDESC.
 *
 * All or nothing.  need_bytes > cap_bytes: USN_DV_OVERFLOW_BYTES; every
 * metadata array and need_bytes are valid and complete and no byte of `frames`
 * is written.  USN_DR_BADDESC: what was written stays inside frames[0,
 * min(need_bytes, cap_bytes)) and is unspecified.  In both cases NO HEAD MOVES
 * and taken = 0.  Otherwise every byte of frames[0, need_bytes) is written,
 * nothing past it, head[e] += take[e] and taken = selected.  frames, lens, src,
 * pos16, tail and btail of the set are never written.
 *
 * The heads move in the call's LAST launch, after every unit they release has
 * been read.  The call must still be stream-ordered with the appends
 * (usn_deliver_brings) and head updates (usn_bringset_set_head) of the same
 * set: the plan reads the counters in the first launch.
 *
 * Every index is clamped (desc_off / unit_off to the totals, take to D, nu to
 * B, a descriptor by & (D - 1), a unit by & (B - 1), output positions to cap /
 * cap_bytes): whatever the counters, lens or pos16 hold, no access leaves the
 * set or the drain. */
#define USN_HAS_BRINGS_DRAIN 1
#define USN_BDRAIN_UTILE 4096 /* 16-byte units per copy tile of usn_brings_drain (one workgroup, four passes) */
#define USN_DR_BADDESC 64u    /* usn_brings_drain: a selected ring's pos16 / lens chain is inconsistent: no head moved */
/* Three launches on `hip_stream` (plan, copy, commit); no host synchronisation
 * and no copy in the steady state.  USN_EINVAL: a null pointer, a set that is
 * not ready, a drain that was not bound; USN_ENODEV: a USN_HOST_ONLY context. */
int usn_brings_drain(usn_ctx *ctx, usn_bringset *rs, usn_drain *d, void *hip_stream);
/* Synchronises `hip_stream` and copies the header to the host: USN_ERANGE when
 * USN_DV_OVERFLOW_BYTES, USN_DR_BADCOUNT or USN_DR_BADDESC is set (host_out is
 * filled all the same); USN_DR_MORE alone returns 0. */
int usn_brings_drain_info(usn_ctx *ctx, const usn_drain *d, void *hip_stream, usn_drain_hdr *host_out);

/* Forget the carried decision cache of one endpoint (last_pkt = None). */
int usn_cache_clear(usn_ctx *ctx, uint16_t endpoint);

/* ---- device plumbing for hosts without their own HIP bindings -------------------- */
int usn_dev_alloc(usn_ctx *ctx, size_t bytes, void **dev);
int usn_dev_free(usn_ctx *ctx, void *dev);
int usn_host_alloc_pinned(usn_ctx *ctx, size_t bytes, void **host);
int usn_host_free_pinned(usn_ctx *ctx, void *host);
int usn_memcpy_h2d(usn_ctx *ctx, void *dev, const void *host, size_t bytes, void *hip_stream);
int usn_memcpy_d2h(usn_ctx *ctx, void *host, const void *dev, size_t bytes, void *hip_stream);
int usn_memset_d(usn_ctx *ctx, void *dev, int value, size_t bytes, void *hip_stream);
int usn_stream_create(usn_ctx *ctx, void **stream);
int usn_stream_destroy(usn_ctx *ctx, void *stream);
int usn_stream_sync(usn_ctx *ctx, void *stream);
int usn_device_sync(usn_ctx *ctx);
/* Events: elapsed milliseconds between two recorded events. */
int usn_event_create(usn_ctx *ctx, void **ev);
int usn_event_destroy(usn_ctx *ctx, void *ev);
int usn_event_record(usn_ctx *ctx, void *ev, void *hip_stream);
int usn_event_elapsed_ms(usn_ctx *ctx, void *ev_start, void *ev_end, float *ms);
/* Make `hip_stream` wait (on the device) for an event recorded on another stream. */
int usn_stream_wait_event(usn_ctx *ctx, void *hip_stream, void *ev);

#ifdef __cplusplus
}
#endif
#endif /* USN_CLASSIFY_H */
