// Save / load of ONE Raft or CRaft replica object's state on the device: the canonical image and its two kernels.
// (included by raft_engine.hip behind RaftView / CraftView)
//
// A snapshot holds what the replica's next handler call depends on: what the reference writes into and reads back from its
// snapshot file and WAL (raft/snapshot.rs, raft/recovery.rs recover_from_wal, craft/snapshot.rs) plus the volatile state its
// crash-restart loop (summerset_server/src/main.rs:124-167) loses and a checkpoint must not -- role, votes, the leader's
// per-peer indices, the CRaft heartbeat counters and the queued Reconstruct slots.  It is the logical state and nothing of the
// arena's layout: a replica's window does not show in it as long as its ring has dropped no entry (ring_lo equal); once a
// smaller ring has moved ring_lo the logical states differ (the dumps do too) and so may the bytes.
// Not carried: wire_acc (zero between calls), ring rows outside the live span (load leaves them alone, the dumps give zero
// there) and the CRaft payload store's shard bytes (smr_craft_pstore_*: a restored replica's store is refilled by follow /
// Reconstruct as after any restart).
// Chosen groups (smr_raft_save_groups / smr_raft_load_groups / smr_raft_reset_groups and their cluster forms) go through the
// same image and the same bodies: an image of "these n groups, in this order" is the image of an n-group replica, read and
// written through a group list (SnapGroupList below).  A group image holds zero counters, and like every image none of
// the CRaft payload store's shard bytes.
//
// Image (little-endian; every section starts on a multiple of 8; padding bytes are zero):
//   RaftSnapHdr                                      64 B
//   counters u64[8]                                  commits, redirects, rejects, entries sent, reconstruct_data calls, postponed
//                                                    executions, ring-guard hits, spare -- summed over their 256 shards
//   scalars, structure-of-arrays over groups         curr_term u64[G]; log_len, start_slot, last_commit, last_snap, ring_lo,
//                                                    n_exec, n_trunc u32[G]; next_slot, try_next_slot, match_slot u32[R][G]
//                                                    (row `me` zero); role, leader, voted_for, votes u8[G]; padded to 8
//   CRaft only                                       hb_replied, hb_seen u64[R][G]; last_recon, rq_n u32[G]; hb_repeat u8[R][G];
//                                                    full_copy, alive, partial u8[G]; padded to 8
//   entry_term u64[n_entries]                        tile-major (64 groups), then row k = slot - lo, then group: the groups of
//                                                    a row that hold a k-th live entry, packed -- a wavefront's stores of a row
//                                                    are one contiguous piece
//   CRaft only: RaftSnapRq[n_rq]                     the Reconstruct queue, the same order, row = queue position
//   CRaft only: entry_mask u8[n_entries]             the order of entry_term; padded to 8
// ring_lo is stored as what it stands for, max(ring_lo, log_len - W) (raft_live_lo): the image then tells its live spans
// without the window it came from.  On the device the record sections sit at fixed capacities behind the fixed part; export
// closes the gaps.
#pragma once
#include "snapshot_common.h"

namespace smr {

constexpr uint32_t RSNAP_MAGIC = 0x53465253u;      // "SRFS"
constexpr uint32_t RSNAP_VERSION = 1;
constexpr uint32_t RSNAP_MAX_LOG = 1u << 20;        // no window is larger

struct RaftSnapHdr {
    uint32_t magic, version;
    uint32_t n_groups; uint8_t population, me, commit_extra, variant;      // variant: 0 plain Raft, 1 CRaft
    uint8_t fault_tolerance, repeat_threshold, reserved0[6];
    uint64_t bytes, n_entries, n_rq;
    uint32_t max_live, max_rq;
    uint64_t reserved1;
};
struct RaftSnapRq { uint64_t term; uint32_t slot, pad; };
static_assert(sizeof(RaftSnapHdr) == 64 && sizeof(RaftSnapRq) == 16, "image records");

// ---- the one place that knows which entries of a log are live (shared with smr_raft_leader_dump and
// smr_raft_craft_dump_masks): [max(start_slot, ring_lo, log_len > W ? log_len - W : 0), log_len), empty when truncation left
// log_len below it
SMR_HD uint32_t raft_ring_lo(uint32_t rlo, uint32_t len, uint32_t W) { return (len > W && len - W > rlo) ? len - W : rlo; }
SMR_HD uint32_t raft_live_lo(uint32_t start, uint32_t rlo, uint32_t len, uint32_t W) {
    const uint32_t lo = raft_ring_lo(rlo, len, W);
    return start > lo ? start : lo;
}
SMR_HD uint32_t raft_live_n(uint32_t start, uint32_t rlo, uint32_t len, uint32_t W) {
    const uint32_t lo = raft_live_lo(start, rlo, len, W);
    return len > lo ? len - lo : 0u;
}

// ---- where things are in an image ---------------------------------------------------------------------------------------
struct RaftSnapGeom {
    uint32_t G, R, craft;
    SnapTiles tiles;
    uint64_t off_ctr, off_scal, off_craft, fixed;
    uint64_t o_term, o_len, o_start, o_commit, o_snap, o_rlo, o_nexec, o_ntrunc, o_next, o_try, o_match, o_role, o_leader, o_voted, o_votes, scal_end;
    uint64_t c_hbr, c_hbs, c_lrecon, c_rqn, c_hbrep, c_full, c_alive, c_partial, craft_end;
};
SMR_HD RaftSnapGeom rsnap_geom(uint32_t G, uint32_t R, bool craft) {
    RaftSnapGeom q;
    q.G = G; q.R = R; q.craft = craft ? 1u : 0u; q.tiles = snap_tiles(G);
    const uint64_t g = G, gr = (uint64_t)G * R;
    q.off_ctr = sizeof(RaftSnapHdr);
    q.off_scal = q.off_ctr + 8 * 8;
    q.o_term = 0; q.o_len = 8 * g; q.o_start = 12 * g; q.o_commit = 16 * g; q.o_snap = 20 * g; q.o_rlo = 24 * g; q.o_nexec = 28 * g;
    q.o_ntrunc = 32 * g; q.o_next = 36 * g; q.o_try = q.o_next + 4 * gr; q.o_match = q.o_try + 4 * gr;
    q.o_role = q.o_match + 4 * gr; q.o_leader = q.o_role + g; q.o_voted = q.o_leader + g; q.o_votes = q.o_voted + g;
    q.scal_end = q.o_votes + g;
    q.off_craft = q.off_scal + snap_a8(q.scal_end);
    q.c_hbr = 0; q.c_hbs = 8 * gr; q.c_lrecon = 16 * gr; q.c_rqn = q.c_lrecon + 4 * g; q.c_hbrep = q.c_rqn + 4 * g;
    q.c_full = q.c_hbrep + gr; q.c_alive = q.c_full + g; q.c_partial = q.c_alive + g; q.craft_end = q.c_partial + g;
    q.fixed = q.off_craft + (craft ? snap_a8(q.craft_end) : 0);
    return q;
}
// one replica's image on the device: the fixed part, then room for cap_e entry terms, cap_rq queue records, cap_e masks
struct RaftSnapImg {
    uint8_t *base;
    uint64_t cap_e, cap_rq;
};
SMR_HD uint64_t rsnap_off_rq(const RaftSnapGeom &q, const RaftSnapImg &S) { return q.fixed + S.cap_e * 8; }
SMR_HD uint64_t rsnap_off_mask(const RaftSnapGeom &q, const RaftSnapImg &S) { return rsnap_off_rq(q, S) + S.cap_rq * sizeof(RaftSnapRq); }
SMR_HD uint64_t rsnap_dev_bytes(const RaftSnapGeom &q, const RaftSnapImg &S) { return rsnap_off_mask(q, S) + (q.craft ? snap_a8(S.cap_e) : 0); }
SMR_HD uint64_t rsnap_bytes(const RaftSnapGeom &q, uint64_t n_e, uint64_t n_rq) {
    return q.fixed + n_e * 8 + (q.craft ? n_rq * sizeof(RaftSnapRq) + snap_a8(n_e) : 0);
}

// the scalar arrays inside an image
struct RaftSnapScal {
    uint64_t *term;
    uint32_t *len, *start, *commit, *snap, *rlo, *nexec, *ntrunc, *next, *tryn, *match;
    uint8_t *role, *leader, *voted, *votes;
    uint64_t *hbr, *hbs;
    uint32_t *lrecon, *rqn;
    uint8_t *hbrep, *full, *alive, *partial;
};
SMR_HD RaftSnapScal rsnap_scal(uint8_t *base, const RaftSnapGeom &q) {
    uint8_t *b = base + q.off_scal, *c = base + q.off_craft;
    RaftSnapScal s;
    s.term = (uint64_t *)(b + q.o_term);
    s.len = (uint32_t *)(b + q.o_len); s.start = (uint32_t *)(b + q.o_start); s.commit = (uint32_t *)(b + q.o_commit);
    s.snap = (uint32_t *)(b + q.o_snap); s.rlo = (uint32_t *)(b + q.o_rlo); s.nexec = (uint32_t *)(b + q.o_nexec);
    s.ntrunc = (uint32_t *)(b + q.o_ntrunc); s.next = (uint32_t *)(b + q.o_next); s.tryn = (uint32_t *)(b + q.o_try);
    s.match = (uint32_t *)(b + q.o_match);
    s.role = b + q.o_role; s.leader = b + q.o_leader; s.voted = b + q.o_voted; s.votes = b + q.o_votes;
    s.hbr = (uint64_t *)(c + q.c_hbr); s.hbs = (uint64_t *)(c + q.c_hbs);
    s.lrecon = (uint32_t *)(c + q.c_lrecon); s.rqn = (uint32_t *)(c + q.c_rqn);
    s.hbrep = c + q.c_hbrep; s.full = c + q.c_full; s.alive = c + q.c_alive; s.partial = c + q.c_partial;
    return s;
}

// ---- what a new replica object holds for a group ----------------------------------------------------------------------
// The one place that says it: smr_raft_leader_create and smr_raft_craft_enable fill their arrays from here, and
// smr_raft_reset_groups (the unpack of nothing, below) returns a listed group to the same values -- the state right after
// become_the_leader (leadership.rs:145-218) on a log that holds only the dummy entry: role, leader = the replica's own id,
// curr_term = the term it was created with, nobody voted for, log_len / next_slot / try_next_slot as below, every other word
// of the group (its other scalars, match_slot, all W ring rows, the counters of the variant's queue) RAFT_INIT_WORD.  CRaft
// on top: reply_cnts (1, 0, 0) for every peer (heartbeat.rs:117-119) and (0, 0, 0) for the replica itself, every peer alive
// (heartbeat.rs:131), and every ring row's shard bitmap full (the dummy entry and whatever a log holds: every shard).
constexpr uint32_t RAFT_INIT_WORD = 0;
constexpr uint8_t RAFT_INIT_ROLE = ROLE_LEADER, RAFT_INIT_VOTED = NO_REP;
constexpr uint32_t RAFT_INIT_LOG_LEN = 1, RAFT_INIT_NEXT = 1, RAFT_INIT_TRY_NEXT = 1;
SMR_HD uint64_t craft_init_hb_replied(bool peer) { return peer ? 1ull : 0ull; }
SMR_HD uint8_t craft_init_bits(uint32_t R) { return (uint8_t)((1u << R) - 1u); }   // alive, and a ring row's shard bitmap
static_assert(RAFT_INIT_WORD == 0, "create fills bytes");

// ---- which group of the replica an image position holds: snapshot_common.h's SnapAllGroups / SnapGroupList -----------------
// What a group image does not carry (WHOLE = false): the eight counters.  The image's counters are zero, and a load through a
// list leaves the target's alone.

// ---- the kernels --------------------------------------------------------------------------------------------------------
// blockIdx.y = which replica of the call (the single calls are the cluster form with n = 1); the replicas are reached
// through the device copies of their views, as smr_raft_cluster_replicate's followers are.  Tiles, bases and placement are
// snapshot_common.h's; a group's counts cost the bases 12 to 16 B out of the L2.
struct RaftSnapArgs {
    const RaftView *rv[RMAX];
    const CraftView *cv[RMAX];
    uint8_t *img[RMAX];
    uint64_t cap_e[RMAX], cap_rq[RMAX];
    uint8_t commit_extra[RMAX];
    RaftSnapGeom geo;
};
// what the listed-groups kernels take on top: the list (one for all replicas of the call) and, for a reset, the term each
// replica was created with
struct RaftSnapGroups {
    const uint32_t *list;
    uint64_t init_term[RMAX];
};

// live entries and queued Reconstruct slots in front of a wavefront, over image positions: the replica's own (PACK: of the
// group the map puts there) or the image's
template <bool PACK, class Map>
__device__ __forceinline__ void rsnap_bases(const RaftView &v, const CraftView &cv, bool craft, const RaftSnapScal &sc, const Map &M, const SnapWave &w,
                                            uint64_t (&base)[2], uint32_t (&mx)[2]) {
    snap_bases(
        [&](uint32_t x, uint64_t (&add)[2], uint32_t (&m)[2]) {
            uint32_t ne, nq;
            if (PACK) {
                const uint32_t g = M.group(x, true);
                ne = raft_live_n(v.start_slot[g], v.ring_lo[g], v.log_len[g], v.W);
                nq = craft ? cv.rq_n[g] : 0u;
            } else {
                ne = raft_live_n(sc.start[x], sc.rlo[x], sc.len[x], RSNAP_MAX_LOG);
                if (ne > v.W) ne = v.W;                          // (load has refused such an image: max_live <= window)
                nq = craft ? sc.rqn[x] : 0u;
            }
            if (nq > CRAFT_RQ) nq = CRAFT_RQ;
            add[0] += ne; add[1] += nq; m[0] = ne > m[0] ? ne : m[0]; m[1] = nq > m[1] ? nq : m[1];
        },
        w.gb0, w.gw0, base, mx);
}

// the replica of this block: views in registers, the image's descriptor
struct RaftSnapSel {
    RaftView v;
    CraftView cv;
    RaftSnapImg S;
    uint32_t commit_extra;
};
__device__ __forceinline__ RaftSnapSel rsnap_select(const RaftSnapArgs &A) {
    const RaftView *rvp = nullptr;
    const CraftView *cvp = nullptr;
    RaftSnapSel s;
    s.S.base = nullptr; s.S.cap_e = 0; s.S.cap_rq = 0; s.commit_extra = 0;
#pragma unroll
    for (int k = 0; k < (int)RMAX; k++)
        if (blockIdx.y == (unsigned)k) {
            rvp = A.rv[k]; cvp = A.cv[k]; s.S.base = A.img[k]; s.S.cap_e = A.cap_e[k]; s.S.cap_rq = A.cap_rq[k]; s.commit_extra = A.commit_extra[k];
        }
    s.v = *rvp;                                              // copies in registers
    if (A.geo.craft) s.cv = *cvp; else s.cv = CraftView{};
    return s;
}

// save: the whole replica (raft_snap_pack) or the listed groups (raft_snap_pack_groups).  x: the lane's position in the
// image (stride nx), g: its group in the replica (stride G)
template <class Map>
__device__ __forceinline__ void rsnap_pack_all(const RaftSnapArgs &A, const Map &M) {
    const RaftSnapGeom &Q = A.geo;
    const RaftSnapSel X = rsnap_select(A);
    const RaftView &v = X.v;
    const CraftView &cv = X.cv;
    const RaftSnapImg &S = X.S;
    const bool craft = Q.craft != 0;
    const RaftSnapScal sc = rsnap_scal(S.base, Q);
    const uint32_t nx = M.n(v.G, Q.G);
    const SnapWave w = snap_wave(Q.tiles, nx);
    const size_t G = v.G, NX = nx;
    uint64_t base[2];                                            // entries, queue records in front
    uint32_t mx[2];
    rsnap_bases<true>(v, cv, craft, sc, M, w, base, mx);
    uint64_t *const terms = (uint64_t *)(S.base + Q.fixed);
    RaftSnapRq *const rqs = (RaftSnapRq *)(S.base + rsnap_off_rq(Q, S));
    uint8_t *const masks = S.base + rsnap_off_mask(Q, S);
    for (uint32_t t = w.t0; t < w.t1; t++) {
        const uint32_t x = t * 64 + w.lane;
        const bool in = x < nx;
        const uint32_t g = M.group(x, in);
        uint32_t n = 0, lo = 0, nq = 0;
        if (in) {
            const uint32_t len = v.log_len[g], start = v.start_slot[g], rlo = raft_ring_lo(v.ring_lo[g], len, v.W);
            lo = raft_live_lo(start, rlo, len, v.W); n = len > lo ? len - lo : 0u;
            sc.term[x] = v.curr_term[g]; sc.len[x] = len; sc.start[x] = start; sc.commit[x] = v.last_commit[g]; sc.snap[x] = v.last_snap[g];
            sc.rlo[x] = rlo; sc.nexec[x] = v.n_exec[g]; sc.ntrunc[x] = v.n_trunc[g];
            sc.role[x] = v.role[g]; sc.leader[x] = v.leader[g]; sc.voted[x] = v.voted_for[g]; sc.votes[x] = v.votes[g];
            for (uint32_t p = 0; p < v.R; p++) {
                const size_t o = (size_t)p * G + g, i = (size_t)p * NX + x;
                const bool peer = p != v.me;
                sc.next[i] = peer ? v.next_slot[o] : 0u; sc.tryn[i] = peer ? v.try_next_slot[o] : 0u; sc.match[i] = peer ? v.match_slot[o] : 0u;
            }
            if (craft) {
                nq = cv.rq_n[g];
                if (nq > CRAFT_RQ) nq = CRAFT_RQ;
                sc.full[x] = cv.full_copy[g]; sc.alive[x] = cv.alive[g]; sc.partial[x] = cv.partial[g];
                sc.lrecon[x] = cv.last_recon[g]; sc.rqn[x] = nq;
                for (uint32_t p = 0; p < v.R; p++) {
                    const size_t o = (size_t)p * G + g, i = (size_t)p * NX + x;
                    sc.hbr[i] = cv.hb_replied[o]; sc.hbs[i] = cv.hb_seen[o]; sc.hbrep[i] = cv.hb_repeat[o];
                }
            }
        }
        const uint32_t maxn = snap_place(n, base[0], S.cap_e, w.lane, [&](uint32_t k, uint64_t pos) {
            const size_t i = (size_t)((lo + k) & v.Wmask) * G + g;
            terms[pos] = v.entry_term[i];
            if (craft) masks[pos] = v.entry_mask[i];
        });
        const uint32_t maxq = snap_place(nq, base[1], S.cap_rq, w.lane, [&](uint32_t j, uint64_t pos) {
            const size_t i = (size_t)j * G + g;
            RaftSnapRq e;
            e.term = cv.rq_term[i]; e.slot = cv.rq_slot[i]; e.pad = 0;
            rqs[pos] = e;
        });
        mx[0] = maxn > mx[0] ? maxn : mx[0]; mx[1] = maxq > mx[1] ? maxq : mx[1];
    }
    if (Map::WHOLE) snap_counters_save<(int)SMR_CTR_STRIDE>(v.counters, (uint64_t *)(S.base + Q.off_ctr));
    else if (blockIdx.x == 0 && threadIdx.x < 8) ((uint64_t *)(S.base + Q.off_ctr))[threadIdx.x] = 0;   // a group image carries no counters
    if (w.last && w.lane == 0) {                                 // the wavefront of the last tile knows the totals
        RaftSnapHdr h;
        h.magic = RSNAP_MAGIC; h.version = RSNAP_VERSION;
        h.n_groups = nx; h.population = (uint8_t)v.R; h.me = (uint8_t)v.me; h.commit_extra = (uint8_t)X.commit_extra; h.variant = craft ? 1 : 0;
        h.fault_tolerance = craft ? (uint8_t)cv.ft : (uint8_t)0; h.repeat_threshold = craft ? (uint8_t)cv.rep_thr : (uint8_t)0;
        for (int k = 0; k < 6; k++) h.reserved0[k] = 0;
        h.n_entries = base[0]; h.n_rq = base[1]; h.bytes = rsnap_bytes(Q, base[0], base[1]);
        h.max_live = mx[0]; h.max_rq = mx[1]; h.reserved1 = 0;
        *(RaftSnapHdr *)S.base = h;
        snap_zero_pad(S.base, Q.off_scal, Q.scal_end);           // padding is zero
        if (craft) {
            snap_zero_pad(S.base, Q.off_craft, Q.craft_end);
            snap_zero_pad(S.base, rsnap_off_mask(Q, S), base[0] < S.cap_e ? base[0] : S.cap_e);
        }
    }
}

// Load re-establishes: every scalar and peer row (row `me` as smr_raft_leader_create leaves it), the live entries' ring rows,
// ring_lo for THIS window, the counters as one shard (the whole replica only), the whole Reconstruct queue.  Ring rows outside
// the live span keep what they held: no handler reads them (RaftLane::term_at, the leader's rlo guards) and the dumps give
// zero there.
// FRESH: the unpack of nothing -- no image is read, the listed groups become what smr_raft_leader_create and
// smr_raft_craft_enable leave (RAFT_INIT_* above), all W ring rows and the queue's rows included, which is how
// smr_raft_reset_groups empties a slot
template <class Map, bool FRESH>
__device__ __forceinline__ void rsnap_unpack_all(const RaftSnapArgs &A, const Map &M, uint64_t init_term) {
    const RaftSnapGeom &Q = A.geo;
    const RaftSnapSel X = rsnap_select(A);
    const RaftView &v = X.v;
    const CraftView &cv = X.cv;
    const RaftSnapImg &S = X.S;
    const bool craft = Q.craft != 0;
    const RaftSnapScal sc = rsnap_scal(S.base, Q);
    const uint32_t nx = M.n(v.G, Q.G);
    const SnapWave w = snap_wave(Q.tiles, nx);
    const size_t G = v.G, NX = nx;
    uint64_t base[2] = {0, 0};
    uint32_t mx[2];
    if (!FRESH) rsnap_bases<false>(v, cv, craft, sc, M, w, base, mx);
    const uint64_t *const terms = (const uint64_t *)(S.base + Q.fixed);
    const RaftSnapRq *const rqs = (const RaftSnapRq *)(S.base + rsnap_off_rq(Q, S));
    const uint8_t *const masks = S.base + rsnap_off_mask(Q, S);
    for (uint32_t t = w.t0; t < w.t1; t++) {
        const uint32_t x = t * 64 + w.lane;
        const bool in = x < nx;
        const uint32_t g = M.group(x, in);
        uint32_t n = 0, lo = 0, nq = 0;
        if (in && FRESH) {
            v.curr_term[g] = init_term; v.log_len[g] = RAFT_INIT_LOG_LEN; v.start_slot[g] = RAFT_INIT_WORD; v.last_commit[g] = RAFT_INIT_WORD;
            v.last_snap[g] = RAFT_INIT_WORD; v.ring_lo[g] = RAFT_INIT_WORD; v.n_exec[g] = RAFT_INIT_WORD; v.n_trunc[g] = RAFT_INIT_WORD;
            v.role[g] = RAFT_INIT_ROLE; v.leader[g] = (uint8_t)v.me; v.voted_for[g] = RAFT_INIT_VOTED; v.votes[g] = (uint8_t)RAFT_INIT_WORD;
            for (uint32_t p = 0; p < v.R; p++) {
                const size_t o = (size_t)p * G + g;
                v.next_slot[o] = RAFT_INIT_NEXT; v.try_next_slot[o] = RAFT_INIT_TRY_NEXT; v.match_slot[o] = RAFT_INIT_WORD;
            }
            for (uint32_t k = 0; k < v.W; k++) {
                v.entry_term[(size_t)k * G + g] = RAFT_INIT_WORD;
                if (craft) v.entry_mask[(size_t)k * G + g] = craft_init_bits(v.R);
            }
            if (craft) {
                cv.full_copy[g] = (uint8_t)RAFT_INIT_WORD; cv.alive[g] = craft_init_bits(v.R); cv.partial[g] = (uint8_t)RAFT_INIT_WORD;
                cv.last_recon[g] = RAFT_INIT_WORD; cv.rq_n[g] = RAFT_INIT_WORD;
                for (uint32_t p = 0; p < v.R; p++) {
                    const size_t o = (size_t)p * G + g;
                    cv.hb_replied[o] = craft_init_hb_replied(p != v.me); cv.hb_seen[o] = RAFT_INIT_WORD; cv.hb_repeat[o] = (uint8_t)RAFT_INIT_WORD;
                }
                for (uint32_t j = 0; j < CRAFT_RQ; j++) { cv.rq_term[(size_t)j * G + g] = RAFT_INIT_WORD; cv.rq_slot[(size_t)j * G + g] = RAFT_INIT_WORD; }
            }
        }
        if (in && !FRESH) {
            const uint32_t len = sc.len[x], start = sc.start[x], rlo = sc.rlo[x];
            lo = raft_live_lo(start, rlo, len, RSNAP_MAX_LOG); n = len > lo ? len - lo : 0u;
            if (n > v.W) { lo += n - v.W; n = v.W; }              // (refused by the host: max_live <= window)
            v.curr_term[g] = sc.term[x]; v.log_len[g] = len; v.start_slot[g] = start; v.last_commit[g] = sc.commit[x]; v.last_snap[g] = sc.snap[x];
            v.ring_lo[g] = raft_ring_lo(rlo, len, v.W); v.n_exec[g] = sc.nexec[x]; v.n_trunc[g] = sc.ntrunc[x];
            v.role[g] = sc.role[x]; v.leader[g] = sc.leader[x]; v.voted_for[g] = sc.voted[x]; v.votes[g] = sc.votes[x];
            for (uint32_t p = 0; p < v.R; p++) {
                const size_t o = (size_t)p * G + g, i = (size_t)p * NX + x;
                const bool peer = p != v.me;
                v.next_slot[o] = peer ? sc.next[i] : RAFT_INIT_NEXT; v.try_next_slot[o] = peer ? sc.tryn[i] : RAFT_INIT_TRY_NEXT;
                v.match_slot[o] = peer ? sc.match[i] : RAFT_INIT_WORD;
            }
            if (craft) {
                nq = sc.rqn[x];
                if (nq > CRAFT_RQ) nq = CRAFT_RQ;
                cv.full_copy[g] = sc.full[x]; cv.alive[g] = sc.alive[x]; cv.partial[g] = sc.partial[x];
                cv.last_recon[g] = sc.lrecon[x]; cv.rq_n[g] = nq;
                for (uint32_t p = 0; p < v.R; p++) {
                    const size_t o = (size_t)p * G + g, i = (size_t)p * NX + x;
                    cv.hb_replied[o] = sc.hbr[i]; cv.hb_seen[o] = sc.hbs[i]; cv.hb_repeat[o] = sc.hbrep[i];
                }
            }
        }
        if (FRESH) continue;
        snap_place(n, base[0], S.cap_e, w.lane, [&](uint32_t k, uint64_t pos) {
            const size_t i = (size_t)((lo + k) & v.Wmask) * G + g;
            v.entry_term[i] = terms[pos];
            if (craft) v.entry_mask[i] = masks[pos];
        });
        snap_place(nq, base[1], S.cap_rq, w.lane, [&](uint32_t j, uint64_t pos) {
            const size_t i = (size_t)j * G + g;
            const RaftSnapRq e = rqs[pos];
            cv.rq_term[i] = e.term; cv.rq_slot[i] = e.slot;
        });
    }
    if (Map::WHOLE) snap_counters_load<(int)SMR_CTR_STRIDE>((const uint64_t *)(S.base + Q.off_ctr), v.counters);
}

__global__ __launch_bounds__(256) void raft_snap_pack(const RaftSnapArgs A) { rsnap_pack_all(A, SnapAllGroups{}); }
__global__ __launch_bounds__(256) void raft_snap_unpack(const RaftSnapArgs A) { rsnap_unpack_all<SnapAllGroups, false>(A, SnapAllGroups{}, 0); }
// group x of the image (A.geo.G = n groups) <-> group list[x] of the replica; fresh: no image, the listed groups as a new
// replica object holds them (A carries the geometry of n groups and no buffers)
__global__ __launch_bounds__(256) void raft_snap_pack_groups(const RaftSnapArgs A, const RaftSnapGroups L) { rsnap_pack_all(A, SnapGroupList{L.list}); }
__global__ __launch_bounds__(256) void raft_snap_unpack_groups(const RaftSnapArgs A, const RaftSnapGroups L, int fresh) {
    uint64_t term = 0;
#pragma unroll
    for (int k = 0; k < (int)RMAX; k++) if (blockIdx.y == (unsigned)k) term = L.init_term[k];
    if (fresh) rsnap_unpack_all<SnapGroupList, true>(A, SnapGroupList{L.list}, term);
    else rsnap_unpack_all<SnapGroupList, false>(A, SnapGroupList{L.list}, term);
}

}  // namespace smr
