// Save / load of ONE EPaxos replica object's state on the device: the canonical image and its two kernels.
// (included by ep_engine.hip behind EpView / EpExec)
//
// A snapshot holds what the replica's next handler call or host read depends on, in the canonical form the four host dumps define
// (smr_ep_dump, smr_ep_xp_dump, smr_ep_exec_dump, smr_ep_exec_poll): what they report for a cell or a scalar is what the image
// carries, plus the stored PreAcceptReplies and the executor's commit-bar copies, which no dump shows and the next handler reads.
// Nothing of the arena's layout goes in: not the 32-bit KV word (ep_kv_pack: the image holds the reference's 64-bit tokens), not the
// per-key table's stride (hc_es / hc_kv: a replica seated in a cluster's shared table and an unseated one give the same bytes),
// not sq32 (load recomputes it), not ring residues (the unpolled submissions are (row, column) pairs).
//
// Image (little-endian; every section starts on a multiple of 8; padding bytes are zero; DESIGN.md 2 has the table):
//   EpSnapHdr                                        64 B
//   counters u64[7]                                  EpView::counters, summed over their shards
//   counters u64[8]              (execute)           EpExec::counters (slot 3, the "column >= 2^28" count, goes along: a loaded
//                                                    replica goes on answering SMR_ERR_STATE where the saved one did)
//   scalars, structure-of-arrays over groups,        len, commit_bars u32[R][G]; rewritten u8[G]; with execute exec_bars, prev_cb
//   each array padded to 8                           u32[R][G], digest u64[G], n_sub u32[G]; highest_cols u32[n_keys][R][G]; with
//                                                    execute kv u64[n_keys][G] (tokens)
//   (zero to the next multiple of 16)
//   EpSnapCell[n_cells]                              64 B each, one per live cell; tile-major (64 groups), then row, then
//                                                    k = column - first live column, then group: the groups of the tile that hold
//                                                    such a cell, packed
//   reply records [n_replies]                        one per live cell of the rows that have reply tables -- my row, every row with
//                                                    recovery -- in the order of those cells; a fixed stride (epsnap_geom)
//   exec entries {u32 col, u32 row}[n_exec]          the unpolled submissions: tile-major, then list position, then group
// The live span of row r of a group is [len > W ? len - W : 0, len) (ep_live_lo, shared with the dumps).  There is no ring_lo
// beside len, so an image loads only into a replica of the window it came from.
//
// What is reachable in the reply tables (the canonical rule; everything else is 0 / SMR_EP_NONE in the image):
//   - peer p's PreAcceptReply (pa_seq, pa_deps) of a cell: where the cell has leader bookkeeping (bk bit 0), is PreAccepting and
//     bit p of pa_acks is set.  Every reader -- EpLaneT::pre_accept_reply, ep_pa_replies_lane_rd, the ballot-0 re-evaluation of
//     ep_heartbeat_timeout_kernel -- returns before the table unless Status == PreAccepting and bk & 1, and loads behind
//     `on = (acks >> p) & 1`.  PreAccepting is part of the rule, not only the ack bit: ep_pa_replies_lane_rd sets the ack bits of
//     the replies that decided an instance without storing them ("the replies of a decided instance are not stored"), so behind
//     a set bit of an instance that has left PreAccepting lies whatever the ring cell's previous occupant left.
//   - peer p's exp_prepare_voteds entry (xv_status, xv_key, xv_seq, xv_deps): where the cell has leader bookkeeping and bit p of
//     the has-entry bits is set (EpLaneT::exp_prepare_reply loads behind `on = (has >> p) & 1`; smr_ep_xp_dump's rule).
//   exp_prepare_max_bal, exp_prepare_acks and the has-entry bits read as zero without leader bookkeeping (smr_ep_xp_dump), and
//   all four explicit-prepare fields are zero without recovery.
//
// Not carried:
//   - ring cells outside the live span: load leaves them alone.  Every reader guards on len (EpLaneT::held; max_seq_num and
//     ep_propose_lane look at sq32 / p0 only behind held(); the executor's walk pops a cell only if held; the dumps give null
//     cells there).
//   - my_nulls: derived.  Load recounts it as the Null cells of my row's live span.  (The engine's own count never forgets a
//     Null cell that left the span, so it can be larger; only "!= 0" is ever read, and with no Null cell in the span the scan it
//     allows finds nothing.)
//   - the executor's graph arrays node_of / nslot / head / sib / parent: zero or dead between two attempts, and every attempt
//     ends inside the handler call that started it.
//   - wire_acc (the wire call's cumulative scratch) and word 7 of the engine's counter shards (smr_ep_cluster_batch_stats:
//     measurement, not state; load zeroes it).
//   - anything of smr_ep_cluster / smr_ep_spread: the reply stacks, flag arrays and defer lists are written before they are
//     read inside every tick (a tick counts its deferred lanes into the block of its `parity` and empties the other block for
//     the next tick; a cluster object made later starts with both empty), and the cluster's shared per-key table is reached through the replica's own view.
#pragma once
#include "snapshot_common.h"

namespace smr {

constexpr uint32_t EPSNAP_MAGIC = 0x53504553u;      // "SEPS"
constexpr uint32_t EPSNAP_VERSION = 1;
constexpr uint32_t EPSNAP_MAX_WINDOW = 1u << 15;     // population * window <= 32768 with execution; no larger window is needed

struct EpSnapHdr {
    uint32_t magic, version;
    uint64_t bytes;
    uint32_t n_groups; uint8_t population, me, optimized_quorum, execute, recovery, reserved0[3];
    uint32_t window, n_keys, max_live;
    uint64_t n_cells, n_exec;
    uint32_t max_exec;
    uint32_t n_replies;                                          // (below 2^28: a record plane of the replica stays under 4 GB)
};
struct EpSnapCell {                                              // four 16-byte words
    uint64_t bal, seq;                                           //   = p0
    uint32_t deps[8];                                            //   deps[0..3] = p1; SMR_EP_NONE at and above R
    uint64_t xp_max;                                             //   exp_prepare_max_bal
    uint8_t status, key, bk, pa_acks, acc_acks, avoid, xp_acks, xp_has;   // = the engine's meta words m0, m1
};
struct EpSnapExec { uint32_t col, row; };
static_assert(sizeof(EpSnapHdr) == 64 && sizeof(EpSnapCell) == 64 && sizeof(EpSnapExec) == 8, "image records");

// ---- the one place that knows which cells of a row are live (shared with the dumps): [len > W ? len - W : 0, len)
SMR_HD uint32_t ep_live_lo(uint32_t len, uint32_t W) { return len > W ? len - W : 0u; }
SMR_HD uint32_t ep_live_n(uint32_t len, uint32_t W) { return len - ep_live_lo(len, W); }
// ... and the column ring cell w of that row holds, if any (W a power of two)
SMR_HD bool ep_live_col(uint32_t len, uint32_t W, uint32_t w, uint32_t &col) {
    const uint32_t lo = ep_live_lo(len, W);
    col = (lo & ~(W - 1u)) | w;
    if (col < lo) col += W;
    return col < len;
}

// ---- where things are in an image ---------------------------------------------------------------------------------------
struct EpSnapGeom {
    uint32_t G, R, K, execute, recovery;
    SnapTiles tiles;
    uint64_t off_ctr, o_len, o_cb, o_rew, o_eb, o_pcb, o_digest, o_nsub, o_hc, o_kv, o_end, fixed;   // fixed: o_end on a multiple of 16
    // a reply record: pa_seq u64[R]; xv_seq u64[R] (recovery); pa_deps u32[R][R]; xv_deps u32[R][R], xv_status u8[R],
    // xv_key u8[R] (recovery); padded to 8
    uint32_t r_xq, r_pd, r_xd, r_xs, r_xk, r_end, r_stride;
};
SMR_HD EpSnapGeom epsnap_geom(uint32_t G, uint32_t R, uint32_t K, uint32_t execute, uint32_t recovery) {
    EpSnapGeom q;
    q.G = G; q.R = R; q.K = K; q.execute = execute; q.recovery = recovery; q.tiles = snap_tiles(G);
    const uint64_t g = G, rg4 = snap_a8(4 * g * R);
    q.off_ctr = sizeof(EpSnapHdr);
    q.o_len = q.off_ctr + 8 * (7 + (execute ? 8 : 0));
    q.o_cb = q.o_len + rg4; q.o_rew = q.o_cb + rg4;
    q.o_eb = q.o_rew + snap_a8(g);
    q.o_pcb = q.o_eb + (execute ? rg4 : 0); q.o_digest = q.o_pcb + (execute ? rg4 : 0);
    q.o_nsub = q.o_digest + (execute ? 8 * g : 0);
    q.o_hc = q.o_nsub + (execute ? snap_a8(4 * g) : 0);
    q.o_kv = q.o_hc + snap_a8(4 * g * R * K);
    q.o_end = q.o_kv + (execute ? 8 * g * K : 0);
    q.fixed = snap_a16(q.o_end);                                 // the cell records are moved as 16-byte words
    q.r_xq = 8 * R; q.r_pd = q.r_xq + (recovery ? 8 * R : 0); q.r_xd = q.r_pd + 4 * R * R;
    q.r_xs = q.r_xd + (recovery ? 4 * R * R : 0); q.r_xk = q.r_xs + (recovery ? R : 0); q.r_end = q.r_xk + (recovery ? R : 0);
    q.r_stride = (uint32_t)snap_a8(q.r_end);
    return q;
}
// one replica's image on the device: the fixed part, then room for cap_c cell records, cap_r reply records, cap_x exec entries
struct EpSnapImg {
    uint8_t *base;
    uint64_t cap_c, cap_r, cap_x;
};
SMR_HD uint64_t epsnap_off_rep(const EpSnapGeom &q, const EpSnapImg &S) { return q.fixed + S.cap_c * sizeof(EpSnapCell); }
SMR_HD uint64_t epsnap_off_exec(const EpSnapGeom &q, const EpSnapImg &S) { return epsnap_off_rep(q, S) + S.cap_r * q.r_stride; }
SMR_HD uint64_t epsnap_dev_bytes(const EpSnapGeom &q, const EpSnapImg &S) { return epsnap_off_exec(q, S) + S.cap_x * sizeof(EpSnapExec); }
SMR_HD uint64_t epsnap_bytes(const EpSnapGeom &q, uint64_t n_c, uint64_t n_r, uint64_t n_x) {
    return q.fixed + n_c * sizeof(EpSnapCell) + n_r * q.r_stride + n_x * sizeof(EpSnapExec);
}

// the scalar arrays inside an image (those of the executor only with execute)
struct EpSnapScal {
    uint32_t *len, *cb, *eb, *pcb, *nsub, *hc;
    uint8_t *rew;
    uint64_t *digest, *kv;
};
SMR_HD EpSnapScal epsnap_scal(uint8_t *b, const EpSnapGeom &q) {
    EpSnapScal s;
    s.len = (uint32_t *)(b + q.o_len); s.cb = (uint32_t *)(b + q.o_cb); s.rew = b + q.o_rew;
    s.eb = (uint32_t *)(b + q.o_eb); s.pcb = (uint32_t *)(b + q.o_pcb); s.digest = (uint64_t *)(b + q.o_digest);
    s.nsub = (uint32_t *)(b + q.o_nsub); s.hc = (uint32_t *)(b + q.o_hc); s.kv = (uint64_t *)(b + q.o_kv);
    return s;
}

// ---- what a new replica object holds for a group ------------------------------------------------------------------------
// The one place that says it: smr_ep_replica_create's ep_init_records_kernel fills the record planes from here, and
// smr_ep_reset_groups (the unpack of nothing, below) returns a listed group to the same values.  Every word of a group is
// EP_INIT_WORD (its scalars, p0, sq32, xp_max, my_nulls, n_sub, the KV word of its per-key entries) except: the dependencies of
// every ring cell are none and its key is none -- all R * W ring cells are null instances (EpInst::make_null) -- and the
// highest columns of its per-key entries are none.
constexpr uint32_t EP_INIT_WORD = 0;
__device__ __forceinline__ u32x4 ep_init_p0() { return (u32x4){EP_INIT_WORD, EP_INIT_WORD, EP_INIT_WORD, EP_INIT_WORD}; }
__device__ __forceinline__ u32x4 ep_init_p1() { return (u32x4){EP_NONE, EP_NONE, EP_NONE, EP_NONE}; }
__device__ __forceinline__ u32x4 ep_init_p2() { return (u32x4){EP_NONE, (uint32_t)EP_NO_KEY << 8, EP_INIT_WORD, EP_NONE}; }
__device__ __forceinline__ u32x4 ep_init_p3() { return (u32x4){EP_NONE, EP_NONE, EP_INIT_WORD, EP_INIT_WORD}; }
static_assert(EP_INIT_WORD == 0, "create fills the arena with zero bytes");

// ---- which group of the replica an image position holds: snapshot_common.h's SnapAllGroups / SnapGroupList -----------------
// Chosen groups (smr_ep_save_groups / smr_ep_load_groups / smr_ep_reset_groups and their cluster forms) go through the same
// image and the same bodies: an image of "these n groups, in this order" is the version-1 image of an n-group replica whose
// group x is group list[x] of this one.  The image's side of every index is the position x with stride n (the scalar arrays,
// the tiles, the bases, the placement); the object's side is the group g = list[x] with stride G (the view's and the executor's
// arrays, the per-key entry (g * K + k) * hc_es at the view's own hc_es / hc_kv, order[j * G + g]).
// What travels with a group is everything the image rules above cover.  What does not (WHOLE = false): the seven engine and eight
// executor counters -- a group image holds zero counters and a load through a list leaves the target's alone, word 7 of the
// shards (batch_stats) included, so sums over objects are conserved -- and, as for the whole object, ring cells outside the
// live span, wire_acc and anything of smr_ep_cluster / smr_ep_spread.
// Reset (FRESH, the unpack of nothing) writes what the list above says, for all R * W ring cells.  It does not write the reply
// tables (pa_seq, pa_deps, xv_*) nor the executor's graph arrays and `order`: nothing reaches a reply-table entry without a
// live cell's leader bookkeeping and ack / has-entry bits (the canonical rule above), the graph arrays are zero or dead
// between two attempts, and `order` is read only below n_sub.

// ---- the kernels --------------------------------------------------------------------------------------------------------
// blockIdx.y = which replica of the call (the single calls are the cluster form with n = 1).  The views travel by value and are
// indexed only by the block-uniform blockIdx.y, so they stay in the kernarg segment.  Tiles, bases and placement
// are snapshot_common.h's; a group's counts cost the bases 4 R (+ 4) bytes out of the L2.
struct EpSnapArgs {
    EpView v[SMR_MAX_REPLICAS];
    EpExec x[SMR_MAX_REPLICAS];
    uint8_t *img[SMR_MAX_REPLICAS];
    uint64_t cap_c[SMR_MAX_REPLICAS], cap_r[SMR_MAX_REPLICAS], cap_x[SMR_MAX_REPLICAS];
    uint8_t oq[SMR_MAX_REPLICAS];                                // smr_ep_cfg.optimized_quorum (the view holds only the quorum sizes)
    EpSnapGeom geo;                                              // the image's: of the snapshot's groups
};

// live cells and unpolled submissions in front of a wavefront, over image positions: the replica's own (PACK: of the group the
// map puts there) or the image's (of the same window: the host has refused any other).  base[0] holds two counts, the live
// cells of every row in its low half and those of my row in its high half -- each stays below 2^28 (smr_ep_replica_create: a
// record plane under 4 GB), and the prefix keeps its 96 bytes of LDS.  NX: the image's groups
template <bool PACK, class Map>
__device__ __forceinline__ void epsnap_bases(const EpView &v, const EpExec &x, const EpSnapGeom &Q, const EpSnapScal &sc, const Map &M, size_t NX,
                                             const SnapWave &w, uint64_t (&base)[2], uint32_t (&mx)[2]) {
    const uint32_t *const len = PACK ? v.len : sc.len, *const nsub = PACK ? x.n_sub : sc.nsub;
    const size_t stride = PACK ? (size_t)v.G : NX;
    snap_bases(
        [&](uint32_t xi, uint64_t (&add)[2], uint32_t (&m)[2]) {
            const uint32_t g = PACK ? M.group(xi, true) : xi;
            uint32_t all = 0, mine = 0;
            for (uint32_t r = 0; r < v.R; r++) {
                const uint32_t n = ep_live_n(len[(size_t)r * stride + g], v.W);
                all += n; mine = r == v.me ? n : mine; m[0] = n > m[0] ? n : m[0];
            }
            uint32_t nx = Q.execute ? nsub[g] : 0u;
            if (nx > 2u * v.R * v.W) nx = 2u * v.R * v.W;        // (the list's capacity: EpExecLaneT::submit_ring)
            add[0] += (uint64_t)all | ((uint64_t)mine << 32); add[1] += nx; m[1] = nx > m[1] ? nx : m[1];
        },
        w.gb0, w.gw0, base, mx);
}

// save: the whole replica (ep_snap_pack) or the listed groups (ep_snap_pack_groups).  xi: the lane's position in the image
// (stride NX), g: its group in the replica (stride G).  The lanes behind the last position stay in every wave-wide step and
// contribute nothing: their group reads as 0, their loads are safe and their stores guarded by `on`
template <class Map>
__device__ __forceinline__ void epsnap_pack_all(const EpSnapArgs &A, const Map &M) {
    const EpSnapGeom &Q = A.geo;
    const uint32_t rep = blockIdx.y < SMR_MAX_REPLICAS ? blockIdx.y : 0u;
    const EpView &v = A.v[rep];
    const EpExec &x = A.x[rep];
    const EpSnapImg S{A.img[rep], A.cap_c[rep], A.cap_r[rep], A.cap_x[rep]};
    const EpSnapScal sc = epsnap_scal(S.base, Q);
    const uint32_t ni = M.n(v.G, Q.G);
    const SnapWave w = snap_wave(Q.tiles, ni);
    const size_t G = v.G, NX = ni;
    const uint32_t R = v.R, W = v.W, K = v.n_keys, rec = v.recovery, wshift = 31u - (uint32_t)__clz((int)W);
    uint64_t base[2];
    uint32_t mx[2];
    epsnap_bases<true>(v, x, Q, sc, M, NX, w, base, mx);
    uint64_t rbase = rec ? (base[0] & 0xFFFFFFFFull) : (base[0] >> 32);   // reply records in front
    base[0] &= 0xFFFFFFFFull;                                             // cell records in front
    u32x4 *const cells = (u32x4 *)(S.base + Q.fixed);
    uint8_t *const reps = S.base + epsnap_off_rep(Q, S);
    EpSnapExec *const execs = (EpSnapExec *)(S.base + epsnap_off_exec(Q, S));
    for (uint32_t t = w.t0; t < w.t1; t++) {
        const uint32_t xi = t * 64 + w.lane;
        const bool on = xi < ni;
        const uint32_t g = M.group(xi, on);
        uint32_t nx = 0;
        if (on) {
            for (uint32_t r = 0; r < R; r++) {
                const size_t o = (size_t)r * G + g, oi = (size_t)r * NX + xi;
                sc.len[oi] = v.len[o]; sc.cb[oi] = v.commit_bars[o];
                if (Q.execute) { sc.eb[oi] = x.exec_bars[o]; sc.pcb[oi] = x.prev_cb[o]; }
            }
            sc.rew[xi] = v.rewritten[g] ? 1 : 0;
            if (Q.execute) {
                nx = x.n_sub[g];
                if (nx > 2u * R * W) nx = 2u * R * W;
                sc.digest[xi] = x.digest[g]; sc.nsub[xi] = nx;
            }
            for (uint32_t k = 0; k < K; k++) {                   // my entries of the per-key table, wherever the view keeps them
                const uint32_t *const e = v.hc + ((size_t)g * K + k) * v.hc_es;
                for (uint32_t r = 0; r < R; r++) sc.hc[((size_t)k * R + r) * NX + xi] = e[r];
                if (Q.execute) sc.kv[(size_t)k * NX + xi] = ep_kv_unpack(e[v.hc_kv]);
            }
        }
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t len = on ? v.len[(size_t)r * G + g] : 0u, lo = ep_live_lo(len, W);
            const bool tab = rec || r == v.me;                   // this row has reply tables
            const uint64_t b0 = base[0];
            const uint32_t maxn = snap_place(len - lo, base[0], S.cap_c, w.lane, [&](uint32_t k, uint64_t pos) {
                const uint32_t wc = (lo + k) & v.Wmask;
                const size_t i = ((size_t)r * W + wc) * G + g;
                const u32x4 a = v.p0[i], b = v.p1[i], c = v.p2[i];
                u32x4 d = (u32x4){R > 4 ? c.x : EP_NONE, R > 5 ? c.w : EP_NONE, EP_NONE, EP_NONE};
                if (R > 6) { const u32x4 e = v.p3[i]; d.z = e.x; d.w = R > 7 ? e.y : EP_NONE; }
                const uint32_t m0 = c.y;
                const bool lbk = (m0 >> 16) & 1u;
                const uint32_t m1 = !rec ? (c.z & 0xFFu) : lbk ? c.z : (c.z & 0xFFFFu);
                const uint64_t xm = (rec && lbk) ? v.xp_max[i] : 0ull;
                cells[pos * 4] = a;
                cells[pos * 4 + 1] = (u32x4){b.x, b.y, b.z, R > 3 ? b.w : EP_NONE};
                cells[pos * 4 + 2] = d;
                cells[pos * 4 + 3] = (u32x4){(uint32_t)xm, (uint32_t)(xm >> 32), m0, m1};
                const uint64_t rpos = rec ? pos : rbase + (pos - b0);
                if (!tab || rpos >= S.cap_r) return;
                uint8_t *const q = reps + rpos * Q.r_stride;
                const uint32_t acks = (lbk && (m0 & 0xFFu) == EST_PREACCEPTING) ? m0 >> 24 : 0u, has = lbk ? m1 >> 24 : 0u;
                const size_t pw = (size_t)(rec ? r : 0u) * W + wc;
                for (uint32_t p = 0; p < R; p++) {
                    const bool pa = (acks >> p) & 1u, xv = (has >> p) & 1u;
                    const size_t o = (pw * R + p) * G + g;
                    ((uint64_t *)q)[p] = pa ? v.pa_seq[o] : 0ull;
                    for (uint32_t j = 0; j < R; j++) ((uint32_t *)(q + Q.r_pd))[p * R + j] = pa ? v.pa_deps[((pw * R + p) * R + j) * G + g] : EP_NONE;
                    if (!rec) continue;
                    ((uint64_t *)(q + Q.r_xq))[p] = xv ? v.xv_seq[o] : 0ull;
                    q[Q.r_xs + p] = xv ? v.xv_status[o] : 0; q[Q.r_xk + p] = xv ? v.xv_key[o] : EP_NO_KEY;
                    for (uint32_t j = 0; j < R; j++) ((uint32_t *)(q + Q.r_xd))[p * R + j] = xv ? v.xv_deps[((pw * R + p) * R + j) * G + g] : EP_NONE;
                }
                for (uint32_t p = Q.r_end; p < Q.r_stride; p++) q[p] = 0;
            });
            if (!rec && r == v.me) rbase += base[0] - b0;
            mx[0] = maxn > mx[0] ? maxn : mx[0];
        }
        const uint32_t maxx = snap_place(nx, base[1], S.cap_x, w.lane, [&](uint32_t j, uint64_t pos) {
            const uint32_t ring = x.order[(size_t)j * G + g], row = (ring >> wshift) < R ? ring >> wshift : 0u;
            uint32_t col;
            (void)ep_live_col(v.len[(size_t)row * G + g], W, ring & v.Wmask, col);
            execs[pos] = EpSnapExec{col, row};
        });
        mx[1] = maxx > mx[1] ? maxx : mx[1];
    }
    if (Map::WHOLE) {
        snap_counters_save<7>(v.counters, (uint64_t *)(S.base + Q.off_ctr));
        if (Q.execute) snap_counters_save<8>(x.counters, (uint64_t *)(S.base + Q.off_ctr) + 7);
    } else if (blockIdx.x == 0 && threadIdx.x < 7u + (Q.execute ? 8u : 0u)) {
        ((uint64_t *)(S.base + Q.off_ctr))[threadIdx.x] = 0;     // a group image carries no counters
    }
    if (w.last && w.lane == 0) {                                 // the wavefront of the last tile knows the totals
        if (rec) rbase = base[0];
        EpSnapHdr h;
        h.magic = EPSNAP_MAGIC; h.version = EPSNAP_VERSION;
        h.bytes = epsnap_bytes(Q, base[0], rbase, base[1]);
        h.n_groups = ni; h.population = (uint8_t)R; h.me = (uint8_t)v.me;
        h.optimized_quorum = A.oq[rep];
        h.execute = (uint8_t)Q.execute; h.recovery = (uint8_t)rec;
        h.reserved0[0] = h.reserved0[1] = h.reserved0[2] = 0;
        h.window = W; h.n_keys = K; h.max_live = mx[0];
        h.n_cells = base[0]; h.n_exec = base[1]; h.max_exec = mx[1]; h.n_replies = (uint32_t)rbase;
        *(EpSnapHdr *)S.base = h;
        snap_zero_pad(S.base, Q.o_len, 4 * NX * R); snap_zero_pad(S.base, Q.o_cb, 4 * NX * R); snap_zero_pad(S.base, Q.o_rew, NX);
        if (Q.execute) { snap_zero_pad(S.base, Q.o_eb, 4 * NX * R); snap_zero_pad(S.base, Q.o_pcb, 4 * NX * R); snap_zero_pad(S.base, Q.o_nsub, 4 * NX); }
        snap_zero_pad(S.base, Q.o_hc, 4 * NX * R * K);
        for (uint64_t p = Q.o_end; p < Q.fixed; p++) S.base[p] = 0;
    }
}

// Load re-establishes, every one from the image's values: every scalar; the live cells' records at column & Wmask, with sq32 =
// min(seq, 2^32 - 1) beside p0 and m0 / m1 repacked; xp_max; the reply tables' entries of those cells; the per-key entries at the
// view's own hc_es / hc_kv (a replica seated in a cluster's shared table loads into its slots of that table) with the KV word
// through ep_kv_pack; my_nulls recounted; order / n_sub as ring cells of this replica; the counters as one shard (the whole
// replica only).
// FRESH: the unpack of nothing -- no image is read, the listed groups become what smr_ep_replica_create leaves (EP_INIT_* above),
// all R * W ring cells included, which is how smr_ep_reset_groups empties a slot
template <class Map, bool FRESH>
__device__ __forceinline__ void epsnap_unpack_all(const EpSnapArgs &A, const Map &M) {
    const EpSnapGeom &Q = A.geo;
    const uint32_t rep = blockIdx.y < SMR_MAX_REPLICAS ? blockIdx.y : 0u;
    const EpView &v = A.v[rep];
    const EpExec &x = A.x[rep];
    const EpSnapImg S{A.img[rep], A.cap_c[rep], A.cap_r[rep], A.cap_x[rep]};
    const EpSnapScal sc = epsnap_scal(S.base, Q);
    const uint32_t ni = M.n(v.G, Q.G);
    const SnapWave w = snap_wave(Q.tiles, ni);
    const size_t G = v.G, NX = ni;
    const uint32_t R = v.R, W = v.W, K = v.n_keys, rec = v.recovery, wshift = 31u - (uint32_t)__clz((int)W);
    uint64_t base[2] = {0, 0};
    uint32_t mx[2];
    if (!FRESH) epsnap_bases<false>(v, x, Q, sc, M, NX, w, base, mx);
    uint64_t rbase = rec ? (base[0] & 0xFFFFFFFFull) : (base[0] >> 32);
    base[0] &= 0xFFFFFFFFull;
    const u32x4 *const cells = (const u32x4 *)(S.base + Q.fixed);
    const uint8_t *const reps = S.base + epsnap_off_rep(Q, S);
    const EpSnapExec *const execs = (const EpSnapExec *)(S.base + epsnap_off_exec(Q, S));
    for (uint32_t t = w.t0; t < w.t1; t++) {
        const uint32_t xi = t * 64 + w.lane;
        const bool on = xi < ni;
        const uint32_t g = M.group(xi, on);
        uint32_t nx = 0, nulls = 0;
        if (on && FRESH) {
            for (uint32_t r = 0; r < R; r++) {
                const size_t o = (size_t)r * G + g;
                v.len[o] = EP_INIT_WORD; v.commit_bars[o] = EP_INIT_WORD;
                if (Q.execute) { x.exec_bars[o] = EP_INIT_WORD; x.prev_cb[o] = EP_INIT_WORD; }
            }
            v.rewritten[g] = (uint8_t)EP_INIT_WORD; v.my_nulls[g] = EP_INIT_WORD;
            if (Q.execute) { x.digest[g] = EP_INIT_WORD; x.n_sub[g] = EP_INIT_WORD; }
            for (uint32_t k = 0; k < K; k++) {
                uint32_t *const e = v.hc + ((size_t)g * K + k) * v.hc_es;
                for (uint32_t r = 0; r < R; r++) e[r] = EP_NONE;
                e[v.hc_kv] = EP_INIT_WORD;
            }
            for (uint32_t c = 0; c < R * W; c++) {               // every ring cell a null instance
                const size_t i = (size_t)c * G + g;
                v.p0[i] = ep_init_p0(); v.sq32[i] = EP_INIT_WORD; v.p1[i] = ep_init_p1(); v.p2[i] = ep_init_p2();
                if (R > 6) v.p3[i] = ep_init_p3();
                if (rec) v.xp_max[i] = EP_INIT_WORD;
            }
        }
        if (FRESH) continue;
        if (on) {
            for (uint32_t r = 0; r < R; r++) {
                const size_t o = (size_t)r * G + g, oi = (size_t)r * NX + xi;
                v.len[o] = sc.len[oi]; v.commit_bars[o] = sc.cb[oi];
                if (Q.execute) { x.exec_bars[o] = sc.eb[oi]; x.prev_cb[o] = sc.pcb[oi]; }
            }
            v.rewritten[g] = sc.rew[xi];
            if (Q.execute) {
                nx = sc.nsub[xi];
                if (nx > 2u * R * W) nx = 2u * R * W;            // (refused by the host)
                x.digest[g] = sc.digest[xi]; x.n_sub[g] = nx;
            }
            for (uint32_t k = 0; k < K; k++) {
                uint32_t *const e = v.hc + ((size_t)g * K + k) * v.hc_es;
                for (uint32_t r = 0; r < R; r++) e[r] = sc.hc[((size_t)k * R + r) * NX + xi];
                if (Q.execute) e[v.hc_kv] = ep_kv_pack(sc.kv[(size_t)k * NX + xi]);
            }
        }
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t len = on ? sc.len[(size_t)r * NX + xi] : 0u, lo = ep_live_lo(len, W);
            const bool tab = rec || r == v.me;
            const uint64_t b0 = base[0];
            snap_place(len - lo, base[0], S.cap_c, w.lane, [&](uint32_t k, uint64_t pos) {
                const uint32_t wc = (lo + k) & v.Wmask;
                const size_t i = ((size_t)r * W + wc) * G + g;
                const u32x4 a = cells[pos * 4], b = cells[pos * 4 + 1], d = cells[pos * 4 + 2], m = cells[pos * 4 + 3];
                v.p0[i] = a;
                v.sq32[i] = a.w ? 0xFFFFFFFFu : a.z;             // min(seq, 2^32 - 1)
                v.p1[i] = b;
                v.p2[i] = (u32x4){d.x, m.z, m.w, d.y};
                if (R > 6) v.p3[i] = (u32x4){d.z, d.w, 0u, 0u};
                if (rec) v.xp_max[i] = (uint64_t)m.x | ((uint64_t)m.y << 32);
                if (r == v.me && (m.z & 0xFFu) == EST_NULL) nulls++;
                const uint64_t rpos = rec ? pos : rbase + (pos - b0);
                if (!tab || rpos >= S.cap_r) return;
                const uint8_t *const q = reps + rpos * Q.r_stride;
                const size_t pw = (size_t)(rec ? r : 0u) * W + wc;
                for (uint32_t p = 0; p < R; p++) {
                    const size_t o = (pw * R + p) * G + g;
                    v.pa_seq[o] = ((const uint64_t *)q)[p];
                    for (uint32_t j = 0; j < R; j++) v.pa_deps[((pw * R + p) * R + j) * G + g] = ((const uint32_t *)(q + Q.r_pd))[p * R + j];
                    if (!rec) continue;
                    v.xv_seq[o] = ((const uint64_t *)(q + Q.r_xq))[p];
                    v.xv_status[o] = q[Q.r_xs + p]; v.xv_key[o] = q[Q.r_xk + p];
                    for (uint32_t j = 0; j < R; j++) v.xv_deps[((pw * R + p) * R + j) * G + g] = ((const uint32_t *)(q + Q.r_xd))[p * R + j];
                }
            });
            if (!rec && r == v.me) rbase += base[0] - b0;
        }
        if (on) v.my_nulls[g] = nulls;
        snap_place(nx, base[1], S.cap_x, w.lane, [&](uint32_t j, uint64_t pos) {
            const EpSnapExec e = execs[pos];
            const uint32_t row = e.row < R ? e.row : 0u;         // (refused by the host)
            x.order[(size_t)j * G + g] = (uint16_t)((row << wshift) | (e.col & v.Wmask));
        });
    }
    if (Map::WHOLE) {
        snap_counters_load<7>((const uint64_t *)(S.base + Q.off_ctr), v.counters);
        if (Q.execute) snap_counters_load<8>((const uint64_t *)(S.base + Q.off_ctr) + 7, x.counters);
    }
}

__global__ __launch_bounds__(256) void ep_snap_pack(const EpSnapArgs A) { epsnap_pack_all(A, SnapAllGroups{}); }
__global__ __launch_bounds__(256) void ep_snap_unpack(const EpSnapArgs A) { epsnap_unpack_all<SnapAllGroups, false>(A, SnapAllGroups{}); }
// group x of the image (A.geo.G = n groups) <-> group list[x] of the replica, one list for all replicas of the call; fresh: no
// image, the listed groups as a new replica object holds them (A carries the geometry of n groups and no buffers)
__global__ __launch_bounds__(256) void ep_snap_pack_groups(const EpSnapArgs A, const uint32_t *list) { epsnap_pack_all(A, SnapGroupList{list}); }
__global__ __launch_bounds__(256) void ep_snap_unpack_groups(const EpSnapArgs A, const uint32_t *list, int fresh) {
    if (fresh) epsnap_unpack_all<SnapGroupList, true>(A, SnapGroupList{list});
    else epsnap_unpack_all<SnapGroupList, false>(A, SnapGroupList{list});
}

}  // namespace smr
