// Save / load of ONE RSPaxos replica object's state on the device: the canonical image and its two kernels.
// (included by rsp_engine.hip behind RspView)
//
// A snapshot holds what the replica's next handler call or host read depends on: what the reference writes into and reads back
// from its snapshot file and WAL (rspaxos/snapshot.rs, rspaxos/recovery.rs) plus the volatile state its crash-restart loop
// (summerset_server/src/main.rs:124-167) loses and a checkpoint must not -- ballots, the leader's and the replica's bookkeeping of
// every live instance, the peers' exec bars, the commands the last handler call executed and the host has not polled yet.  It is
// the logical state in the canonical form smr_rsp_dump defines and nothing of the arena's layout.
// Not carried: ring cells outside the live span (load leaves them alone: every reader guards on len -- RspLane::held, ring_lo --
// and the dump gives null instances there) and the payload store's shard bytes (smr_rsp_pstore_*).
//
// Image (little-endian; every section starts on a multiple of 8; padding bytes are zero):
//   RspSnapHdr                                       64 B
//   counters u64[4]                                  commits, commands executed, mixed absorbs, redirects -- summed over their shards
//   scalars, structure-of-arrays over groups,        leader u8[G]; bal_prep_sent, bal_prepared, bal_max_seen u64[G]; len, commit_bar,
//   each array padded to 8                           exec_bar, snap_bar u32[G]; peer_exec_bar u32[R][G]; digest u64[G]; xn u32[G]
//   RspSnapSlot[n_slots]                             56 B each; tile-major (64 groups), then row k = slot - first live slot, then
//                                                    group: the groups of a tile that hold a k-th live instance, packed -- a
//                                                    wavefront's stores of a row are one contiguous piece
//   exec entries u32[n_exec]                         the slots of the unpolled execution list, the same order, row = list position;
//                                                    padded to 8
// The live span of a group is [len > W ? len - W : 0, len) (rsp_live_lo): a slot is held iff slot + W >= len, there is no ring_lo
// beside len, so an image loads only into a replica of the window it came from.  On the device the record sections sit at fixed
// capacities behind the fixed part; export closes the gaps.
// Chosen groups (smr_rsp_save_groups / smr_rsp_load_groups / smr_rsp_reset_groups and their cluster forms) go through the same
// image and the same bodies: an image of "these n groups, in this order" is the image of an n-group replica, read and written
// through a group list (SnapGroupList below).  A group image holds zero counters; the unpolled execution list is per-group
// rows and travels like every other section.
#pragma once
#include "snapshot_common.h"

namespace smr {

constexpr uint32_t RSPSNAP_MAGIC = 0x53505253u;     // "SRPS"
constexpr uint32_t RSPSNAP_VERSION = 1;
constexpr uint32_t RSPSNAP_MAX_WINDOW = 1u << 20;    // no window is larger

struct RspSnapHdr {
    uint32_t magic, version;
    uint32_t n_groups; uint8_t population, me, fault_tolerance, reserved0;
    uint32_t window, max_live;
    uint64_t bytes, n_slots, n_exec;
    uint32_t max_exec, reserved1;
    uint64_t reserved2;
};
struct RspSnapSlot {
    uint64_t bal, vbal, pmax;
    uint32_t val, vval, ltrig, lendp, rtrig, rendp;
    uint8_t status, mask, vmask, flags, packs, aacks, rsrc, zero;
};
static_assert(sizeof(RspSnapHdr) == 64 && sizeof(RspSnapSlot) == 56, "image records");

// ---- the one place that knows which instances of a log are live (shared with smr_rsp_dump): [len > W ? len - W : 0, len)
SMR_HD uint32_t rsp_live_lo(uint32_t len, uint32_t W) { return len > W ? len - W : 0u; }
SMR_HD uint32_t rsp_live_n(uint32_t len, uint32_t W) { return len - rsp_live_lo(len, W); }
// ... and what an instance's bookkeeping fields read as where it has no such bookkeeping (shared with smr_rsp_dump)
SMR_HD void rsp_slot_canon(RspSnapSlot &s) {
    if (!(s.flags & RFL_LBK)) { s.ltrig = 0; s.lendp = 0; s.packs = 0; s.aacks = 0; s.pmax = 0; }
    if (!(s.flags & RFL_RBK)) { s.rsrc = RSP_NO_REP; s.rtrig = 0; s.rendp = 0; }
}

// ---- where things are in an image ---------------------------------------------------------------------------------------
struct RspSnapGeom {
    uint32_t G, R;
    SnapTiles tiles;
    uint64_t off_ctr, o_leader, o_bps, o_bpd, o_bms, o_len, o_cbar, o_ebar, o_snap, o_peb, o_digest, o_xn, fixed;
};
SMR_HD RspSnapGeom rspsnap_geom(uint32_t G, uint32_t R) {
    RspSnapGeom q;
    q.G = G; q.R = R; q.tiles = snap_tiles(G);
    const uint64_t g = G, g1 = snap_a8(g), g4 = snap_a8(4 * g), g8 = 8 * g;
    q.off_ctr = sizeof(RspSnapHdr);
    q.o_leader = q.off_ctr + 4 * 8;
    q.o_bps = q.o_leader + g1; q.o_bpd = q.o_bps + g8; q.o_bms = q.o_bpd + g8;
    q.o_len = q.o_bms + g8; q.o_cbar = q.o_len + g4; q.o_ebar = q.o_cbar + g4; q.o_snap = q.o_ebar + g4;
    q.o_peb = q.o_snap + g4; q.o_digest = q.o_peb + snap_a8(4 * g * R); q.o_xn = q.o_digest + g8;
    q.fixed = q.o_xn + g4;
    return q;
}
// one replica's image on the device: the fixed part, then room for cap_s slot records and cap_x exec entries
struct RspSnapImg {
    uint8_t *base;
    uint64_t cap_s, cap_x;
};
SMR_HD uint64_t rspsnap_off_exec(const RspSnapGeom &q, const RspSnapImg &S) { return q.fixed + S.cap_s * sizeof(RspSnapSlot); }
SMR_HD uint64_t rspsnap_dev_bytes(const RspSnapGeom &q, const RspSnapImg &S) { return rspsnap_off_exec(q, S) + snap_a8(S.cap_x * 4); }
SMR_HD uint64_t rspsnap_bytes(const RspSnapGeom &q, uint64_t n_s, uint64_t n_x) { return q.fixed + n_s * sizeof(RspSnapSlot) + snap_a8(n_x * 4); }

// the scalar arrays inside an image
struct RspSnapScal {
    uint8_t *leader;
    uint64_t *bps, *bpd, *bms, *digest;
    uint32_t *len, *cbar, *ebar, *snap, *peb, *xn;
};
SMR_HD RspSnapScal rspsnap_scal(uint8_t *b, const RspSnapGeom &q) {
    RspSnapScal s;
    s.leader = b + q.o_leader;
    s.bps = (uint64_t *)(b + q.o_bps); s.bpd = (uint64_t *)(b + q.o_bpd); s.bms = (uint64_t *)(b + q.o_bms); s.digest = (uint64_t *)(b + q.o_digest);
    s.len = (uint32_t *)(b + q.o_len); s.cbar = (uint32_t *)(b + q.o_cbar); s.ebar = (uint32_t *)(b + q.o_ebar); s.snap = (uint32_t *)(b + q.o_snap);
    s.peb = (uint32_t *)(b + q.o_peb); s.xn = (uint32_t *)(b + q.o_xn);
    return s;
}

// ---- what a new replica object holds for a group ----------------------------------------------------------------------
// The one place that says it: smr_rsp_replica_create fills its arrays from here, and smr_rsp_reset_groups (the unpack of
// nothing, below) returns a listed group to the same values -- no leader known, every other word of the group (its scalars, the
// peers' exec bars, the digest, all W ring rows, the execution list's rows) RSP_INIT_WORD, except the two value ids of every ring
// row, which are null.  (smr_rsp_preset_leader is a step after create, not part of it.)
constexpr uint32_t RSP_INIT_WORD = 0;
constexpr uint8_t RSP_INIT_LEADER = RSP_NO_REP;
constexpr uint8_t RSP_INIT_VAL_BYTE = 0xFF;                  // create fills bytes: s_val / s_vval of every ring row
constexpr uint32_t RSP_INIT_VAL = 0x01010101u * RSP_INIT_VAL_BYTE;
static_assert(RSP_INIT_WORD == 0 && RSP_INIT_LEADER == 0xFF, "create fills bytes");

// ---- which group of the replica an image position holds: snapshot_common.h's SnapAllGroups / SnapGroupList -----------------
// What a group image does not carry (WHOLE = false): the four counters.  The image's counters are zero, and a load through a
// list leaves the target's alone.

// ---- the kernels --------------------------------------------------------------------------------------------------------
// blockIdx.y = which replica of the call (the single calls are the cluster form with n = 1).  An RSPaxos replica keeps no device
// copy of its view: the views travel by value and are indexed only by the block-uniform blockIdx.y, so they stay in the kernarg
// segment.  Tiles, bases and placement are snapshot_common.h's; a group's counts cost the bases
// 8 B out of the L2.
struct RspSnapArgs {
    RspView v[SMR_MAX_REPLICAS];
    uint8_t *img[SMR_MAX_REPLICAS];
    uint64_t cap_s[SMR_MAX_REPLICAS], cap_x[SMR_MAX_REPLICAS];
    RspSnapGeom geo;
};

// live instances and unpolled executions in front of a wavefront, over image positions: the replica's own (PACK: of the group
// the map puts there) or the image's (of the same window: the host has refused any other)
template <bool PACK, class Map>
__device__ __forceinline__ void rspsnap_bases(const RspView &v, const RspSnapScal &sc, const Map &M, const SnapWave &w, uint64_t (&base)[2], uint32_t (&mx)[2]) {
    snap_bases(
        [&](uint32_t x, uint64_t (&add)[2], uint32_t (&m)[2]) {
            const uint32_t g = PACK ? M.group(x, true) : x;
            const uint32_t ns = rsp_live_n(PACK ? v.len[g] : sc.len[x], v.W);
            uint32_t nx = PACK ? v.xn[g] : sc.xn[x];
            if (nx > v.W) nx = v.W;                              // (smr_rsp_exec_poll reads no more)
            add[0] += ns; add[1] += nx; m[0] = ns > m[0] ? ns : m[0]; m[1] = nx > m[1] ? nx : m[1];
        },
        w.gb0, w.gw0, base, mx);
}

// save: the whole replica (rsp_snap_pack) or the listed groups (rsp_snap_pack_groups).  x: the lane's position in the image
// (stride ni), g: its group in the replica (stride G)
template <class Map>
__device__ __forceinline__ void rspsnap_pack_all(const RspSnapArgs &A, const Map &M) {
    const RspSnapGeom &Q = A.geo;
    const uint32_t rep = blockIdx.y < SMR_MAX_REPLICAS ? blockIdx.y : 0u;
    const RspView &v = A.v[rep];
    const RspSnapImg S{A.img[rep], A.cap_s[rep], A.cap_x[rep]};
    const RspSnapScal sc = rspsnap_scal(S.base, Q);
    const uint32_t ni = M.n(v.G, Q.G);
    const SnapWave w = snap_wave(Q.tiles, ni);
    const size_t G = v.G, NX = ni;
    uint64_t base[2];                                            // slot records, exec entries in front
    uint32_t mx[2];
    rspsnap_bases<true>(v, sc, M, w, base, mx);
    RspSnapSlot *const recs = (RspSnapSlot *)(S.base + Q.fixed);
    uint32_t *const execs = (uint32_t *)(S.base + rspsnap_off_exec(Q, S));
    for (uint32_t t = w.t0; t < w.t1; t++) {
        const uint32_t x = t * 64 + w.lane;
        const bool in = x < ni;
        const uint32_t g = M.group(x, in);
        uint32_t n = 0, lo = 0, nx = 0;
        if (in) {
            const uint32_t len = v.len[g];
            lo = rsp_live_lo(len, v.W); n = len - lo;
            nx = v.xn[g];
            if (nx > v.W) nx = v.W;
            sc.leader[x] = v.leader[g]; sc.bps[x] = v.bps[g]; sc.bpd[x] = v.bpd[g]; sc.bms[x] = v.bms[g];
            sc.len[x] = len; sc.cbar[x] = v.cbar[g]; sc.ebar[x] = v.ebar[g]; sc.snap[x] = v.snap[g];
            sc.digest[x] = v.digest[g]; sc.xn[x] = nx;
            for (uint32_t p = 0; p < v.R; p++) sc.peb[(size_t)p * NX + x] = v.peb[(size_t)p * G + g];
        }
        const uint32_t maxn = snap_place(n, base[0], S.cap_s, w.lane, [&](uint32_t k, uint64_t pos) {
            const size_t i = (size_t)((lo + k) & v.Wmask) * G + g;
            RspSnapSlot r;
            r.bal = v.s_bal[i]; r.vbal = v.s_vbal[i]; r.pmax = v.s_pmax[i];
            r.val = v.s_val[i]; r.vval = v.s_vval[i]; r.ltrig = v.s_ltrig[i]; r.lendp = v.s_lendp[i]; r.rtrig = v.s_rtrig[i]; r.rendp = v.s_rendp[i];
            r.status = v.s_st[i]; r.mask = v.s_mask[i]; r.vmask = v.s_vmask[i]; r.flags = v.s_fl[i]; r.packs = v.s_packs[i]; r.aacks = v.s_aacks[i];
            r.rsrc = v.s_rsrc[i]; r.zero = 0;
            rsp_slot_canon(r);
            recs[pos] = r;
        });
        const uint32_t maxx = snap_place(nx, base[1], S.cap_x, w.lane, [&](uint32_t j, uint64_t pos) { execs[pos] = v.xq[(size_t)j * G + g]; });
        mx[0] = maxn > mx[0] ? maxn : mx[0]; mx[1] = maxx > mx[1] ? maxx : mx[1];
    }
    if (Map::WHOLE) snap_counters_save<4>(v.counters, (uint64_t *)(S.base + Q.off_ctr));
    else if (blockIdx.x == 0 && threadIdx.x < 4) ((uint64_t *)(S.base + Q.off_ctr))[threadIdx.x] = 0;   // a group image carries no counters
    if (w.last && w.lane == 0) {                                 // the wavefront of the last tile knows the totals
        RspSnapHdr h;
        h.magic = RSPSNAP_MAGIC; h.version = RSPSNAP_VERSION;
        h.n_groups = ni; h.population = (uint8_t)v.R; h.me = (uint8_t)v.me; h.fault_tolerance = (uint8_t)v.ft; h.reserved0 = 0;
        h.window = v.W; h.max_live = mx[0];
        h.n_slots = base[0]; h.n_exec = base[1]; h.bytes = rspsnap_bytes(Q, base[0], base[1]);
        h.max_exec = mx[1]; h.reserved1 = 0; h.reserved2 = 0;
        *(RspSnapHdr *)S.base = h;
        snap_zero_pad(S.base, Q.o_leader, NX);                   // padding is zero
        snap_zero_pad(S.base, Q.o_len, 4 * NX); snap_zero_pad(S.base, Q.o_cbar, 4 * NX); snap_zero_pad(S.base, Q.o_ebar, 4 * NX);
        snap_zero_pad(S.base, Q.o_snap, 4 * NX); snap_zero_pad(S.base, Q.o_peb, 4 * NX * v.R); snap_zero_pad(S.base, Q.o_xn, 4 * NX);
        snap_zero_pad(S.base, rspsnap_off_exec(Q, S), 4 * (base[1] < S.cap_x ? base[1] : S.cap_x));
    }
}

// Load re-establishes: every scalar and peer row, the live instances' ring cells (at slot & Wmask), the unpolled execution
// list, the counters as one shard (the whole replica only).  Ring cells outside the live span keep what they held: no handler
// reads them (RspLane::held, ring_lo) and the dump gives null instances there.
// FRESH: the unpack of nothing -- no image is read, the listed groups become what smr_rsp_replica_create leaves (RSP_INIT_*
// above), all W ring rows and the execution list's rows included, which is how smr_rsp_reset_groups empties a slot
template <class Map, bool FRESH>
__device__ __forceinline__ void rspsnap_unpack_all(const RspSnapArgs &A, const Map &M) {
    const RspSnapGeom &Q = A.geo;
    const uint32_t rep = blockIdx.y < SMR_MAX_REPLICAS ? blockIdx.y : 0u;
    const RspView &v = A.v[rep];
    const RspSnapImg S{A.img[rep], A.cap_s[rep], A.cap_x[rep]};
    const RspSnapScal sc = rspsnap_scal(S.base, Q);
    const uint32_t ni = M.n(v.G, Q.G);
    const SnapWave w = snap_wave(Q.tiles, ni);
    const size_t G = v.G, NX = ni;
    uint64_t base[2] = {0, 0};
    uint32_t mx[2];
    if (!FRESH) rspsnap_bases<false>(v, sc, M, w, base, mx);
    const RspSnapSlot *const recs = (const RspSnapSlot *)(S.base + Q.fixed);
    const uint32_t *const execs = (const uint32_t *)(S.base + rspsnap_off_exec(Q, S));
    for (uint32_t t = w.t0; t < w.t1; t++) {
        const uint32_t x = t * 64 + w.lane;
        const bool in = x < ni;
        const uint32_t g = M.group(x, in);
        uint32_t n = 0, lo = 0, nx = 0;
        if (in && FRESH) {
            v.leader[g] = RSP_INIT_LEADER; v.bps[g] = RSP_INIT_WORD; v.bpd[g] = RSP_INIT_WORD; v.bms[g] = RSP_INIT_WORD;
            v.len[g] = RSP_INIT_WORD; v.cbar[g] = RSP_INIT_WORD; v.ebar[g] = RSP_INIT_WORD; v.snap[g] = RSP_INIT_WORD;
            v.digest[g] = RSP_INIT_WORD; v.xn[g] = RSP_INIT_WORD;
            for (uint32_t p = 0; p < v.R; p++) v.peb[(size_t)p * G + g] = RSP_INIT_WORD;
            for (uint32_t k = 0; k < v.W; k++) {
                const size_t i = (size_t)k * G + g;
                v.s_bal[i] = RSP_INIT_WORD; v.s_vbal[i] = RSP_INIT_WORD; v.s_pmax[i] = RSP_INIT_WORD;
                v.s_val[i] = RSP_INIT_VAL; v.s_vval[i] = RSP_INIT_VAL; v.s_ltrig[i] = RSP_INIT_WORD; v.s_lendp[i] = RSP_INIT_WORD;
                v.s_rtrig[i] = RSP_INIT_WORD; v.s_rendp[i] = RSP_INIT_WORD;
                v.s_st[i] = (uint8_t)RSP_INIT_WORD; v.s_mask[i] = (uint8_t)RSP_INIT_WORD; v.s_vmask[i] = (uint8_t)RSP_INIT_WORD;
                v.s_fl[i] = (uint8_t)RSP_INIT_WORD; v.s_packs[i] = (uint8_t)RSP_INIT_WORD; v.s_aacks[i] = (uint8_t)RSP_INIT_WORD;
                v.s_rsrc[i] = (uint8_t)RSP_INIT_WORD; v.xq[i] = RSP_INIT_WORD;
            }
        }
        if (FRESH) continue;
        if (in) {
            const uint32_t len = sc.len[x];
            lo = rsp_live_lo(len, v.W); n = len - lo;
            nx = sc.xn[x];
            if (nx > v.W) nx = v.W;                              // (refused by the host: max_exec <= window)
            v.leader[g] = sc.leader[x]; v.bps[g] = sc.bps[x]; v.bpd[g] = sc.bpd[x]; v.bms[g] = sc.bms[x];
            v.len[g] = len; v.cbar[g] = sc.cbar[x]; v.ebar[g] = sc.ebar[x]; v.snap[g] = sc.snap[x];
            v.digest[g] = sc.digest[x]; v.xn[g] = nx;
            for (uint32_t p = 0; p < v.R; p++) v.peb[(size_t)p * G + g] = sc.peb[(size_t)p * NX + x];
        }
        snap_place(n, base[0], S.cap_s, w.lane, [&](uint32_t k, uint64_t pos) {
            const size_t i = (size_t)((lo + k) & v.Wmask) * G + g;
            const RspSnapSlot r = recs[pos];
            v.s_bal[i] = r.bal; v.s_vbal[i] = r.vbal; v.s_pmax[i] = r.pmax;
            v.s_val[i] = r.val; v.s_vval[i] = r.vval; v.s_ltrig[i] = r.ltrig; v.s_lendp[i] = r.lendp; v.s_rtrig[i] = r.rtrig; v.s_rendp[i] = r.rendp;
            v.s_st[i] = r.status; v.s_mask[i] = r.mask; v.s_vmask[i] = r.vmask; v.s_fl[i] = r.flags; v.s_packs[i] = r.packs; v.s_aacks[i] = r.aacks;
            v.s_rsrc[i] = r.rsrc;
        });
        snap_place(nx, base[1], S.cap_x, w.lane, [&](uint32_t j, uint64_t pos) { v.xq[(size_t)j * G + g] = execs[pos]; });
    }
    if (Map::WHOLE) snap_counters_load<4>((const uint64_t *)(S.base + Q.off_ctr), v.counters);
}

__global__ __launch_bounds__(256) void rsp_snap_pack(const RspSnapArgs A) { rspsnap_pack_all(A, SnapAllGroups{}); }
__global__ __launch_bounds__(256) void rsp_snap_unpack(const RspSnapArgs A) { rspsnap_unpack_all<SnapAllGroups, false>(A, SnapAllGroups{}); }
// group x of the image (A.geo.G = n groups) <-> group list[x] of the replica, one list for all replicas of the call; fresh: no
// image, the listed groups as a new replica object holds them (A carries the geometry of n groups and no buffers)
__global__ __launch_bounds__(256) void rsp_snap_pack_groups(const RspSnapArgs A, const uint32_t *list) { rspsnap_pack_all(A, SnapGroupList{list}); }
__global__ __launch_bounds__(256) void rsp_snap_unpack_groups(const RspSnapArgs A, const uint32_t *list, int fresh) {
    if (fresh) rspsnap_unpack_all<SnapGroupList, true>(A, SnapGroupList{list});
    else rspsnap_unpack_all<SnapGroupList, false>(A, SnapGroupList{list});
}

}  // namespace smr
