// Save / load of a MultiPaxos cluster's state on the device: the canonical image and its two kernels.
//
// A snapshot holds what the next tick depends on (what the reference writes into and reads back from its snapshot file
// and WAL, snapshot.rs:121-186 / recovery.rs, plus the volatile replica state a crash-restart loop loses and a
// checkpoint must not, summerset_server/src/main.rs:124-167): per live replica the scalars of smr_mp_group_state, every
// slot of [start_slot, log_len) with the fields smr_mp_dump gives, the pending entries of the NEXT tick's outbox, the
// overflow flags, the counters and the committed-slot entries not yet polled.  It is written in ONE canonical form,
// whatever the ring leaves unstored (the ballot run, the follower's meta words), whatever the window, the outbox
// capacity and parity, the straggler list or the way the ticks were launched.
//
// Image (little-endian; every section starts on a multiple of 8; padding bytes are zero), L = live replicas:
//   SnapHdr                                          64 B
//   overflow[G]                                      u8, padded to 8
//   SnapRep[L]                                       counters, commit-list counts
//   L x scalars, structure-of-arrays over groups     bal_prep_sent, bal_prepared, bal_max_seen u64[G]; start_slot,
//                                                    log_len, accept_bar, commit_bar, exec_bar, snap_bar, n_outbox
//                                                    u32[G]; peer_exec_bar u32[R][G]; leader u8[G] padded to 8
//   SnapSlot[n_slots]                                tile-major (64 groups), then replica, then row k = slot -
//                                                    start_slot, then group: the groups of a row that hold a k-th slot,
//                                                    packed -- a wavefront's stores of a row are one contiguous piece
//   SnapMsg[n_outbox]                                the same order, row = outbox entry
//   u64[n_commits]                                   (group << 32) | slot per replica, its groups ascending, a group's
//                                                    entries in commit order
// On the device the three record sections sit at fixed capacities behind the fixed part; export closes the gaps.
#pragma once
#include "mp_device.h"
#include "snapshot_common.h"

namespace smr {

constexpr uint32_t SNAP_MAGIC = 0x53504D53u;      // "SMPS"
constexpr uint32_t SNAP_VERSION = 1;
constexpr uint32_t SNAP_NONE = 0xFFFFFFFFu;

struct SnapHdr {
    uint32_t magic, version;
    uint32_t n_groups; uint8_t population, commit_extra, live_mask, reserved0;
    uint64_t bytes, n_slots, n_outbox, n_commits;
    uint32_t max_live, max_outbox, max_commits, reserved1;
};
struct SnapSlot {                                  // one Instance, explicit (the fields of smr_mp_dump_bufs)
    uint64_t bal, vbal, pmax;
    uint32_t reqs, vreqs, ltrig, lendp, rtrig, rendp;
    uint8_t status, flags, acks, packs, src, pad[3];
};
struct SnapMsg { uint64_t bal; uint32_t slot, val, aux, pad; };   // slot = kind << 30 | slot, as ob_slot
struct SnapRep { uint64_t counters[3], clist_total, clist_carried; };
static_assert(sizeof(SnapHdr) == 64 && sizeof(SnapSlot) == 56 && sizeof(SnapMsg) == 24 && sizeof(SnapRep) == 40, "image records");

// ---- the one place that knows how a ring row reads (shared with smr_mp_dump_range) ------------------------------------
// what slot `slot` holds where the ring leaves it unstored: inside the run [bal_lo, log_len) the ballot is bal_max_seen, a
// follower's meta word is what its append would have stored, and the bars imply the statuses (mp_device.h: Lane::end_run)
SMR_HD void mp_slot_stored(uint32_t slot, uint32_t bal_lo, uint32_t leader, uint32_t rep, uint32_t commit_bar, uint64_t bal_max_seen,
                           uint32_t val, uint64_t &bal, uint32_t &m) {
    if (slot < bal_lo) return;
    bal = bal_max_seen;
    if (leader != rep) m = follower_run_meta(val, leader, slot < commit_bar);
    else if (slot < commit_bar) m = (m & ~M_STATUS) | SMR_ST_EXECUTED;
}
// which side arrays a meta word points into
SMR_HD bool mp_meta_voted_side(uint32_t m) { return ((m >> M_VMODE_SH) & 3u) == VM_SIDE; }
SMR_HD bool mp_meta_lbkx(uint32_t m) { return (m & M_LBK) && (m & M_LBKX); }
SMR_HD bool mp_meta_rbkx(uint32_t m) { return (m & M_RBK) && (m & M_RBKX); }
// meta word + ring values -> explicit Instance fields (side values are read only where the predicates above say so)
SMR_HD SnapSlot mp_slot_canon(uint32_t m, uint64_t bal, uint32_t val, uint64_t vbal, uint32_t vval, uint64_t pmax, uint32_t ltrig,
                              uint32_t lendp, uint32_t rtrig, uint32_t rendp) {
    SnapSlot c;
    const uint32_t vm = (m >> M_VMODE_SH) & 3u;
    const bool lbk = (m & M_LBK) != 0, rbk = (m & M_RBK) != 0, lx = mp_meta_lbkx(m), rx = mp_meta_rbkx(m);
    c.bal = bal; c.reqs = val;
    c.vbal = vm == VM_SAME ? bal : (vm == VM_SIDE ? vbal : 0ull);
    c.vreqs = vm == VM_SAME ? val : (vm == VM_SIDE ? vval : 0u);
    c.pmax = lx ? pmax : 0ull; c.ltrig = lx ? ltrig : 0u; c.lendp = lx ? lendp : 0u;
    c.rtrig = rx ? rtrig : 0u; c.rendp = rx ? rendp : 0u;
    c.status = (uint8_t)(m & M_STATUS);
    c.flags = (uint8_t)((lbk ? 1 : 0) | (rbk ? 2 : 0) | ((m & M_EXT) ? 4 : 0));
    c.acks = lbk ? (uint8_t)((m >> M_ACKS_SH) & 0xFFu) : (uint8_t)0;
    c.packs = lbk ? (uint8_t)((m >> M_PACKS_SH) & 0xFFu) : (uint8_t)0;
    c.src = rbk ? (uint8_t)((m >> M_SRC_SH) & 7u) : (uint8_t)0;
    c.pad[0] = c.pad[1] = c.pad[2] = 0;
    return c;
}
// ... and back: the meta word of an explicit Instance, and which side arrays it needs written
SMR_HD uint32_t mp_slot_meta(const SnapSlot &c, bool &voted_side, bool &lx, bool &rx) {
    uint32_t m = (uint32_t)c.status & M_STATUS;
    if (c.flags & 4) m |= M_EXT;
    lx = rx = false;
    if (c.flags & 1) {
        m |= M_LBK | ((uint32_t)c.acks << M_ACKS_SH) | ((uint32_t)c.packs << M_PACKS_SH);
        lx = c.pmax != 0 || c.ltrig != 0 || c.lendp != 0;
        if (lx) m |= M_LBKX;
    }
    if (c.flags & 2) {
        m |= M_RBK | (((uint32_t)c.src & 7u) << M_SRC_SH);
        rx = c.rtrig != 0 || c.rendp != 0;
        if (rx) m |= M_RBKX;
    }
    if (c.reqs) m |= M_NONEMPTY;
    const uint32_t vm = (c.vbal == c.bal && c.vreqs == c.reqs) ? VM_SAME : ((c.vbal == 0 && c.vreqs == 0) ? VM_NONE : VM_SIDE);
    voted_side = vm == VM_SIDE;
    return m | (vm << M_VMODE_SH);
}

// ---- where things are in an image ---------------------------------------------------------------------------------------
struct SnapGeom {
    uint32_t G, R, live, L;
    SnapTiles tiles;
    uint64_t off_ovf, off_rep, off_scal, scal_stride, fixed;
    uint64_t o_bps, o_bpd, o_bms, o_start, o_len, o_abar, o_cbar, o_ebar, o_snap, o_nob, o_peb, o_leader;
};
SMR_HD SnapGeom snap_geom(uint32_t G, uint32_t R, uint32_t live) {
    SnapGeom q;
    q.G = G; q.R = R; q.live = live; q.L = 0;
    for (uint32_t r = 0; r < R; r++) q.L += (live >> r) & 1u;
    q.tiles = snap_tiles(G);
    const uint64_t g = G;
    q.off_ovf = sizeof(SnapHdr);
    q.off_rep = q.off_ovf + snap_a8(g);
    q.off_scal = q.off_rep + (uint64_t)q.L * sizeof(SnapRep);
    q.o_bps = 0; q.o_bpd = 8 * g; q.o_bms = 16 * g;
    q.o_start = 24 * g; q.o_len = 28 * g; q.o_abar = 32 * g; q.o_cbar = 36 * g; q.o_ebar = 40 * g; q.o_snap = 44 * g; q.o_nob = 48 * g;
    q.o_peb = 52 * g;
    q.o_leader = q.o_peb + 4 * g * R;
    q.scal_stride = snap_a8(q.o_leader + g);
    q.fixed = q.off_scal + (uint64_t)q.L * q.scal_stride;
    return q;
}
struct SnapImg {
    uint8_t *base;
    uint64_t cap_slots, cap_ob, cap_cl;             // records the three sections have room for (device layout)
    SnapGeom geo;
    uint32_t commit_extra;
};
SMR_HD uint64_t snap_off_msgs(const SnapImg &S) { return S.geo.fixed + S.cap_slots * sizeof(SnapSlot); }
SMR_HD uint64_t snap_off_clist(const SnapImg &S) { return snap_off_msgs(S) + S.cap_ob * sizeof(SnapMsg); }
// replica i's (i-th live) scalar arrays inside an image
struct SnapScal {
    uint64_t *bps, *bpd, *bms;
    uint32_t *start, *len, *abar, *cbar, *ebar, *snap, *nob, *peb;
    uint8_t *leader;
};
SMR_HD SnapScal snap_scal(uint8_t *base, const SnapGeom &q, uint32_t i) {
    uint8_t *b = base + q.off_scal + (uint64_t)i * q.scal_stride;
    SnapScal s;
    s.bps = (uint64_t *)(b + q.o_bps); s.bpd = (uint64_t *)(b + q.o_bpd); s.bms = (uint64_t *)(b + q.o_bms);
    s.start = (uint32_t *)(b + q.o_start); s.len = (uint32_t *)(b + q.o_len); s.abar = (uint32_t *)(b + q.o_abar);
    s.cbar = (uint32_t *)(b + q.o_cbar); s.ebar = (uint32_t *)(b + q.o_ebar); s.snap = (uint32_t *)(b + q.o_snap);
    s.nob = (uint32_t *)(b + q.o_nob); s.peb = (uint32_t *)(b + q.o_peb);
    s.leader = b + q.o_leader;
    return s;
}

// ---- which group of the cluster an image position holds: snapshot_common.h's SnapAllGroups / SnapGroupList ------------------
// What a group image does not carry (WHOLE = false): the counters and the unpolled commit list.  They are the cluster's
// reporting, not a group's state: a moved group's unpolled entries stay on the source's list under the source's group id (the
// host polls the source before it reuses the slot).  The image's counters and commit-list words are zero and n_commits = 0; a
// load through a list leaves the target's counters, commit list, straggler list, role_rot and the host's scheduling state alone.

// ---- the kernels --------------------------------------------------------------------------------------------------------
// A wavefront's tiles carry all their live replicas.  Tiles, bases and placement are snapshot_common.h's; a
// group's counts cost the bases 12 B per replica out of the L2.

// live slots and pending outbox entries of replica r (the i-th live one) at image position x: the cluster's own (PACK: of
// the group the map puts there) or the image's
template <bool PACK, class Map>
__device__ __forceinline__ void snap_count(const MpParams &P, int par, const SnapImg &S, const Map &M, uint32_t r, uint32_t i, uint32_t x,
                                           uint32_t &ns, uint32_t &no) {
    if (PACK) {
        const RepView v{P.rep[0], (size_t)r * P.rep_stride};
        const uint32_t g = M.group(x, true);
        ns = v.log_len()[g] - v.start_slot()[g];
        no = v.ob_cnt(par)[g];
    } else {
        const SnapScal sc = snap_scal(S.base, S.geo, i);
        ns = sc.len[x] - sc.start[x];
        no = sc.nob[x];
    }
    if (ns > P.W) ns = P.W;
    if (no > P.cap) no = P.cap;
}

// slot and outbox records of all live replicas in front of a wavefront, and their maxima.  snap_bases' two stages written out,
// replica by replica: with the replicas as the inner loop of snap_bases' per-group functor, save and load of the headline shape
// (65 536 groups x 5 replicas) took 16 % and 22 % longer on the MI355X (profiles/snapshot_refactor_ab.log) -- each replica's
// pass streams through three arrays, and the simple loop over groups is what the compiler keeps several loads in flight for
template <bool PACK, class Map>
__device__ __forceinline__ void mp_snap_bases(const MpParams &P, int par, const SnapImg &S, const Map &M, const SnapWave &w, uint64_t (&base)[2],
                                              uint32_t (&mx)[2]) {
    __shared__ uint64_t sh_s[4], sh_o[4];
    __shared__ uint32_t sh_ms[4], sh_mo[4];
    const uint32_t wv = threadIdx.x >> 6;
    uint64_t s = 0, o = 0;
    uint32_t xs = 0, xo = 0;
    for (uint32_t r = 0, i = 0; r < P.R; r++) {
        if (!((S.geo.live >> r) & 1u)) continue;
        for (uint32_t g = threadIdx.x; g < w.gb0; g += 256) {
            uint32_t ns, no;
            snap_count<PACK>(P, par, S, M, r, i, g, ns, no);
            s += ns; o += no; xs = ns > xs ? ns : xs; xo = no > xo ? no : xo;
        }
        i++;
    }
    s = snap_wave_sum(s); o = snap_wave_sum(o); xs = snap_wave_max(xs); xo = snap_wave_max(xo);
    if (w.lane == 0) { sh_s[wv] = s; sh_o[wv] = o; sh_ms[wv] = xs; sh_mo[wv] = xo; }
    __syncthreads();
    base[0] = sh_s[0] + sh_s[1] + sh_s[2] + sh_s[3];
    base[1] = sh_o[0] + sh_o[1] + sh_o[2] + sh_o[3];
    mx[0] = sh_ms[0]; mx[1] = sh_mo[0];
    for (int k = 1; k < 4; k++) { mx[0] = sh_ms[k] > mx[0] ? sh_ms[k] : mx[0]; mx[1] = sh_mo[k] > mx[1] ? sh_mo[k] : mx[1]; }
    s = 0; o = 0; xs = 0; xo = 0;
    for (uint32_t r = 0, i = 0; r < P.R; r++) {
        if (!((S.geo.live >> r) & 1u)) continue;
        for (uint32_t g = w.gb0 + w.lane; g < w.gw0; g += 64) {
            uint32_t ns, no;
            snap_count<PACK>(P, par, S, M, r, i, g, ns, no);
            s += ns; o += no; xs = ns > xs ? ns : xs; xo = no > xo ? no : xo;
        }
        i++;
    }
    base[0] += snap_wave_sum(s); base[1] += snap_wave_sum(o);
    xs = snap_wave_max(xs); xo = snap_wave_max(xo);
    mx[0] = xs > mx[0] ? xs : mx[0]; mx[1] = xo > mx[1] ? xo : mx[1];
}

// one (tile, replica): scalars, then the slot rows, then the outbox rows.  base: record index of the unit's first slot /
// outbox record on entry, of the next unit's on return.  x: the lane's position in the image, g: its group in the cluster
template <class Map>
__device__ __forceinline__ void snap_pack_unit(const MpParams &P, int par, const SnapImg &S, const Map &M, uint32_t r, uint32_t i, uint32_t tile,
                                               uint64_t (&base)[2], uint32_t (&mx)[2]) {
    const SnapGeom &Q = S.geo;
    const uint32_t lane = threadIdx.x & 63u, x = tile * 64 + lane, nx = M.n(P.G, Q.G);
    const bool in = x < nx;
    const uint32_t g = M.group(x, in);
    const RepView v{P.rep[0], (size_t)r * P.rep_stride};
    const SnapScal sc = snap_scal(S.base, Q, i);
    uint32_t leader = NO_REP, start = 0, len = 0, cbar = 0, brun = SNAP_NONE, nob = 0;
    uint64_t bms = 0;
    if (in) {
        leader = v.leader()[g]; bms = v.bal_max_seen()[g]; start = v.start_slot()[g]; len = v.log_len()[g];
        cbar = v.commit_bar()[g]; brun = v.bal_lo()[g]; nob = v.ob_cnt(par)[g];
        if (nob > P.cap) nob = P.cap;
        sc.leader[x] = (uint8_t)leader; sc.bps[x] = v.bal_prep_sent()[g]; sc.bpd[x] = v.bal_prepared()[g]; sc.bms[x] = bms;
        sc.start[x] = start; sc.len[x] = len; sc.abar[x] = v.accept_bar()[g]; sc.cbar[x] = cbar; sc.ebar[x] = v.exec_bar()[g];
        sc.snap[x] = v.snap_bar()[g]; sc.nob[x] = nob;
        for (uint32_t p = 0; p < P.R; p++) sc.peb[(size_t)p * nx + x] = p == r ? 0u : v.peer_exec_bar()[(size_t)p * P.G + g];
        if (i == 0) S.base[Q.off_ovf + x] = P.overflow[g];
    }
    uint32_t n = in ? len - start : 0u;
    if (n > P.W) n = P.W;
    SnapSlot *const recs = (SnapSlot *)(S.base + Q.fixed);
    const uint32_t maxn = snap_place(n, base[0], S.cap_slots, lane, [&](uint32_t k, uint64_t pos) {
        const uint32_t slot = start + k;
        const size_t t = tix(P.W, slot & P.Wmask, g);
        const uint32_t val = v.s_val()[t];                       // (three independent loads of one row, issued together)
        uint32_t m = v.s_meta()[t];
        uint64_t bal = v.s_bal()[t];
        mp_slot_stored(slot, brun, leader, r, cbar, bms, val, bal, m);
        const bool vs = mp_meta_voted_side(m), lx = mp_meta_lbkx(m), rx = mp_meta_rbkx(m);
        recs[pos] = mp_slot_canon(m, bal, val, vs ? v.s_vbal()[t] : 0ull, vs ? v.s_vval()[t] : 0u, lx ? v.s_pmax()[t] : 0ull,
                                  lx ? v.s_ltrig()[t] : 0u, lx ? v.s_lendp()[t] : 0u, rx ? v.s_rtrig()[t] : 0u, rx ? v.s_rendp()[t] : 0u);
    });
    SnapMsg *const msgs = (SnapMsg *)(S.base + snap_off_msgs(S));
    const uint32_t reg = (in && nob) ? v.ob_reg(par)[g] : 0u;       // a pure append run stores no ob_slot / ob_bal (Lane::ob_end_run)
    const uint64_t rbal = reg ? v.ob_rbal(par)[g] : 0ull;
    const uint32_t maxo = snap_place(nob, base[1], S.cap_ob, lane, [&](uint32_t j, uint64_t pos) {
        const size_t o = tix(P.cap, j, g);
        SnapMsg e;
        e.slot = reg ? ((OB_ACCEPT << OB_KIND_SH) | ((reg - 1 + j) & OB_SLOT_MASK)) : v.ob_slot(par)[o];
        e.bal = reg ? rbal : v.ob_bal(par)[o];
        e.val = v.ob_val(par)[o];
        e.aux = (e.slot >> OB_KIND_SH) == OB_HEARTBEAT ? v.ob_aux(par)[o] : 0u;
        e.pad = 0;
        msgs[pos] = e;
    });
    mx[0] = maxn > mx[0] ? maxn : mx[0]; mx[1] = maxo > mx[1] ? maxo : mx[1];
}

// ... and back.  FRESH: the unpack of nothing -- no image is read, the group becomes what smr_mp_cluster_create leaves
// (mp_types.h: MP_INIT_WORD, MP_INIT_LEADER), which is how smr_mp_reset_groups empties a slot
template <class Map, bool FRESH>
__device__ __forceinline__ void snap_unpack_unit(const MpParams &P, int par, const SnapImg &S, const Map &M, uint32_t r, uint32_t i, uint32_t tile,
                                                 uint64_t (&base)[2]) {
    const SnapGeom &Q = S.geo;
    const uint32_t lane = threadIdx.x & 63u, x = tile * 64 + lane, nx = M.n(P.G, Q.G);
    const bool in = x < nx;
    const uint32_t g = M.group(x, in);
    const RepView v{P.rep[0], (size_t)r * P.rep_stride};
    const SnapScal sc = snap_scal(S.base, Q, i);
    const auto img = [&](const auto *a, size_t k) { return FRESH ? decltype(+a[0])(MP_INIT_WORD) : +a[k]; };
    uint32_t start = 0, len = 0, ebar = 0, nob = 0;
    if (in) {
        start = img(sc.start, x); len = img(sc.len, x); ebar = img(sc.ebar, x); nob = img(sc.nob, x);
        if (nob > P.cap) nob = P.cap;
        v.leader()[g] = FRESH ? (uint8_t)MP_INIT_LEADER : sc.leader[x];
        v.bal_prep_sent()[g] = img(sc.bps, x); v.bal_prepared()[g] = img(sc.bpd, x); v.bal_max_seen()[g] = img(sc.bms, x);
        v.start_slot()[g] = start; v.log_len()[g] = len; v.accept_bar()[g] = img(sc.abar, x); v.commit_bar()[g] = img(sc.cbar, x);
        v.exec_bar()[g] = ebar; v.snap_bar()[g] = img(sc.snap, x);
        for (uint32_t p = 0; p < P.R; p++) v.peer_exec_bar()[(size_t)p * P.G + g] = img(sc.peb, (size_t)p * nx + x);
        // every ballot and meta word below is stored: no run.  The next steady-state append starts one at the log end
        // (BAL_EXTEND, r1_body / r2_body), which is the state every end_run() leaves
        v.bal_lo()[g] = FRESH ? MP_INIT_WORD : SNAP_NONE;
        v.ob_cnt(par)[g] = nob; v.ob_cnt(par ^ 1)[g] = 0;
        v.ob_reg(0)[g] = 0; v.ob_reg(1)[g] = 0;                  // explicit entries
        v.pr_cnt()[g] = 0;
        if (i == 0) { P.overflow[g] = (uint8_t)img(S.base + Q.off_ovf, x); P.r1_done[g] = 0; }
    }
    uint32_t n = in ? len - start : 0u;
    if (n > P.W) n = P.W;
    const SnapSlot *const recs = (const SnapSlot *)(S.base + Q.fixed);
    uint32_t nlb = SNAP_NONE;                                    // first Null at or above exec_bar (MpRep::null_lb), else the log end
    if (!FRESH) snap_place(n, base[0], S.cap_slots, lane, [&](uint32_t k, uint64_t pos) {
        const uint32_t slot = start + k;
        const size_t t = tix(P.W, slot & P.Wmask, g);
        const SnapSlot c = recs[pos];
        bool vs, lx, rx;
        const uint32_t m = mp_slot_meta(c, vs, lx, rx);
        v.s_bal()[t] = c.bal; v.s_val()[t] = c.reqs; v.s_meta()[t] = m;
        if (vs) { v.s_vbal()[t] = c.vbal; v.s_vval()[t] = c.vreqs; }
        if (lx) { v.s_pmax()[t] = c.pmax; v.s_ltrig()[t] = c.ltrig; v.s_lendp()[t] = c.lendp; }
        if (rx) { v.s_rtrig()[t] = c.rtrig; v.s_rendp()[t] = c.rendp; }
        if (nlb == SNAP_NONE && slot >= ebar && (m & M_STATUS) == SMR_ST_NULL) nlb = slot;
    });
    if (in) v.null_lb()[g] = nlb == SNAP_NONE ? len : nlb;
    const SnapMsg *const msgs = (const SnapMsg *)(S.base + snap_off_msgs(S));
    if (!FRESH) snap_place(nob, base[1], S.cap_ob, lane, [&](uint32_t j, uint64_t pos) {
        const size_t o = tix(P.cap, j, g);
        const SnapMsg e = msgs[pos];
        v.ob_slot(par)[o] = e.slot; v.ob_bal(par)[o] = e.bal; v.ob_val(par)[o] = e.val;
        if ((e.slot >> OB_KIND_SH) == OB_HEARTBEAT) v.ob_aux(par)[o] = e.aux;
    });
}

// counters (block 0) and the committed-slot entries not yet polled (the whole grid), replica after replica
template <bool PACK>
__device__ __forceinline__ void snap_lists(const MpParams &P, const SnapImg &S, uint64_t &n_commits, uint32_t &max_commits) {
    const SnapGeom &Q = S.geo;
    unsigned long long *const cl = (unsigned long long *)(S.base + snap_off_clist(S));
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nth = (uint64_t)gridDim.x * 256;
    uint64_t off = 0;
    max_commits = 0;
    for (uint32_t r = 0, i = 0; r < P.R; r++) {
        if (!((Q.live >> r) & 1u)) continue;
        const RepView v{P.rep[0], (size_t)r * P.rep_stride};
        SnapRep *const rp = (SnapRep *)(S.base + Q.off_rep) + i;
        uint64_t total, carried;
        if (PACK) {
            total = *v.clist_n();
            carried = total < P.clist_cap ? total : P.clist_cap;
            for (uint64_t k = tid; k < carried; k += nth)
                if (off + k < S.cap_cl) cl[off + k] = v.clist()[k];
            snap_counters_save<3>(v.counters(), rp->counters);
            if (blockIdx.x == 0 && threadIdx.x == 0) { rp->clist_total = total; rp->clist_carried = carried; }
        } else {
            total = rp->clist_total;
            carried = rp->clist_carried < P.clist_cap ? rp->clist_carried : P.clist_cap;
            for (uint64_t k = tid; k < carried; k += nth)
                if (off + k < S.cap_cl) v.clist()[k] = cl[off + k];
            snap_counters_load<3>(rp->counters, v.counters());   // (and the shards' debug words zero)
            if (blockIdx.x == 0 && threadIdx.x == 0) *v.clist_n() = (unsigned int)total;
        }
        off += carried;
        max_commits = carried > max_commits ? (uint32_t)carried : max_commits;
        i++;
    }
    n_commits = off;
}

// save: the whole cluster (mp_snap_pack) or the listed groups (mp_snap_pack_groups)
template <class Map>
__device__ __forceinline__ void snap_pack_all(const MpParams &P, int par, const SnapImg &S, const Map &M) {
    const SnapGeom &Q = S.geo;
    const uint32_t nx = M.n(P.G, Q.G);
    const SnapWave w = snap_wave(Q.tiles, nx);
    uint64_t base[2];                                            // slot, outbox records in front
    uint32_t mx[2];
    mp_snap_bases<true>(P, par, S, M, w, base, mx);
    for (uint32_t t = w.t0; t < w.t1; t++)
        for (uint32_t r = 0, i = 0; r < P.R; r++) {
            if (!((Q.live >> r) & 1u)) continue;
            snap_pack_unit(P, par, S, M, r, i, t, base, mx);
            i++;
        }
    uint64_t n_commits = 0;
    uint32_t max_commits = 0;
    if (Map::WHOLE) snap_lists<true>(P, S, n_commits, max_commits);
    else if (blockIdx.x == 0 && threadIdx.x < Q.L) {             // a group image carries no counters and no commit entries
        SnapRep z;
        z.counters[0] = z.counters[1] = z.counters[2] = 0; z.clist_total = z.clist_carried = 0;
        ((SnapRep *)(S.base + Q.off_rep))[threadIdx.x] = z;
    }
    if (w.last && w.lane == 0) {                                 // the wavefront of the last tile knows the totals
        SnapHdr h;
        h.magic = SNAP_MAGIC; h.version = SNAP_VERSION;
        h.n_groups = nx; h.population = (uint8_t)P.R; h.commit_extra = (uint8_t)S.commit_extra; h.live_mask = (uint8_t)Q.live; h.reserved0 = 0;
        h.n_slots = base[0]; h.n_outbox = base[1]; h.n_commits = n_commits;
        h.bytes = Q.fixed + base[0] * sizeof(SnapSlot) + base[1] * sizeof(SnapMsg) + n_commits * 8;
        h.max_live = mx[0]; h.max_outbox = mx[1]; h.max_commits = max_commits; h.reserved1 = 0;
        *(SnapHdr *)S.base = h;
        snap_zero_pad(S.base, Q.off_ovf, nx);                    // padding is zero
        for (uint32_t i = 0; i < Q.L; i++) snap_zero_pad(S.base, Q.off_scal + (uint64_t)i * Q.scal_stride, Q.o_leader + nx);
    }
}
// load: the whole cluster (mp_snap_unpack), the listed groups from an image (mp_snap_unpack_groups) or from nothing (FRESH)
template <class Map, bool FRESH>
__device__ __forceinline__ void snap_unpack_all(const MpParams &P, int par, const SnapImg &S, const Map &M) {
    const SnapGeom &Q = S.geo;
    const SnapWave w = snap_wave(Q.tiles, M.n(P.G, Q.G));
    uint64_t base[2] = {0, 0};
    uint32_t mx[2];
    if (!FRESH) mp_snap_bases<false>(P, par, S, M, w, base, mx);
    for (uint32_t t = w.t0; t < w.t1; t++)
        for (uint32_t r = 0, i = 0; r < P.R; r++) {
            if (!((Q.live >> r) & 1u)) continue;
            snap_unpack_unit<Map, FRESH>(P, par, S, M, r, i, t, base);
            i++;
        }
    if (Map::WHOLE) {
        uint64_t n_commits;
        uint32_t max_commits;
        snap_lists<false>(P, S, n_commits, max_commits);
    }
}

__global__ __launch_bounds__(256) void mp_snap_pack(const MpParams *__restrict__ Pp, int par, const SnapImg S) {
    snap_pack_all(*Pp, par, S, SnapAllGroups{});
}
__global__ __launch_bounds__(256) void mp_snap_unpack(const MpParams *__restrict__ Pp, int par, const SnapImg S) {
    snap_unpack_all<SnapAllGroups, false>(*Pp, par, S, SnapAllGroups{});
}
// group i of the image (S.geo.G = n groups) <-> group list[i] of the cluster; fresh: no image, the listed groups as
// smr_mp_cluster_create leaves a group (S carries the geometry of n groups and no buffer)
__global__ __launch_bounds__(256) void mp_snap_pack_groups(const MpParams *__restrict__ Pp, int par, const SnapImg S, const uint32_t *__restrict__ list) {
    snap_pack_all(*Pp, par, S, SnapGroupList{list});
}
__global__ __launch_bounds__(256) void mp_snap_unpack_groups(const MpParams *__restrict__ Pp, int par, const SnapImg S, const uint32_t *__restrict__ list,
                                                             int fresh) {
    if (fresh) snap_unpack_all<SnapGroupList, true>(*Pp, par, S, SnapGroupList{list});
    else snap_unpack_all<SnapGroupList, false>(*Pp, par, S, SnapGroupList{list});
}

}  // namespace smr
