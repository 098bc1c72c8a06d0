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
#pragma once
#include "smr_common.h"

#ifndef SMR_HD
#if defined(__HIPCC__)
#define SMR_HD __host__ __device__ __forceinline__
#else
#define SMR_HD inline
#endif
#endif

namespace smr {

constexpr uint32_t RSPSNAP_MAGIC = 0x53505253u;     // "SRPS"
constexpr uint32_t RSPSNAP_VERSION = 1;
constexpr uint32_t RSPSNAP_MAX_WAVES = 1024;         // wavefronts of a launch per replica; each takes a contiguous piece of the group tiles
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
    uint32_t G, R, ntile, tpw, nwave, nblock;
    uint64_t off_ctr, o_leader, o_bps, o_bpd, o_bms, o_len, o_cbar, o_ebar, o_snap, o_peb, o_digest, o_xn, fixed;
};
SMR_HD uint64_t rspsnap_a8(uint64_t x) { return (x + 7) & ~(uint64_t)7; }
SMR_HD RspSnapGeom rspsnap_geom(uint32_t G, uint32_t R) {
    RspSnapGeom q;
    q.G = G; q.R = R;
    q.ntile = (G + 63) / 64;
    q.tpw = (q.ntile + RSPSNAP_MAX_WAVES - 1) / RSPSNAP_MAX_WAVES;
    q.nwave = (q.ntile + q.tpw - 1) / q.tpw;
    q.nblock = (q.nwave + 3) / 4;
    const uint64_t g = G, g1 = rspsnap_a8(g), g4 = rspsnap_a8(4 * g), g8 = 8 * g;
    q.off_ctr = sizeof(RspSnapHdr);
    q.o_leader = q.off_ctr + 4 * 8;
    q.o_bps = q.o_leader + g1; q.o_bpd = q.o_bps + g8; q.o_bms = q.o_bpd + g8;
    q.o_len = q.o_bms + g8; q.o_cbar = q.o_len + g4; q.o_ebar = q.o_cbar + g4; q.o_snap = q.o_ebar + g4;
    q.o_peb = q.o_snap + g4; q.o_digest = q.o_peb + rspsnap_a8(4 * g * R); q.o_xn = q.o_digest + g8;
    q.fixed = q.o_xn + g4;
    return q;
}
// one replica's image on the device: the fixed part, then room for cap_s slot records and cap_x exec entries
struct RspSnapImg {
    uint8_t *base;
    uint64_t cap_s, cap_x;
};
SMR_HD uint64_t rspsnap_off_exec(const RspSnapGeom &q, const RspSnapImg &S) { return q.fixed + S.cap_s * sizeof(RspSnapSlot); }
SMR_HD uint64_t rspsnap_dev_bytes(const RspSnapGeom &q, const RspSnapImg &S) { return rspsnap_off_exec(q, S) + rspsnap_a8(S.cap_x * 4); }
SMR_HD uint64_t rspsnap_bytes(const RspSnapGeom &q, uint64_t n_s, uint64_t n_x) { return q.fixed + n_s * sizeof(RspSnapSlot) + rspsnap_a8(n_x * 4); }

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

// ---- the kernels --------------------------------------------------------------------------------------------------------
// blockIdx.y = which replica of the call (the single calls are the cluster form with n = 1).  An RSPaxos replica keeps no device
// copy of its view: the views travel by value and are indexed only by the block-uniform blockIdx.y, so they stay in the kernarg
// segment.  Lane = group, a wavefront = a contiguous piece of the 64-group tiles, 4 wavefronts a block.  A
// record's place follows from the live counts of every group in front of it, by the scheme of mp_snapshot.h:
// the block sums the groups in front of its own tiles itself (8 B per group out of the L2: no block waits for another), the
// wavefront adds the tiles of its block in front of its own, and inside a tile a row's records go to the lanes that hold one,
// packed (ballot + prefix count).
struct RspSnapArgs {
    RspView v[SMR_MAX_REPLICAS];
    uint8_t *img[SMR_MAX_REPLICAS];
    uint64_t cap_s[SMR_MAX_REPLICAS], cap_x[SMR_MAX_REPLICAS];
    RspSnapGeom geo;
};

__device__ __forceinline__ uint64_t rspsnap_wave_sum(uint64_t x) {
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ uint32_t rspsnap_wave_max(uint32_t x) {
    for (int off = 32; off > 0; off >>= 1) { const uint32_t y = __shfl_xor(x, off); x = y > x ? y : x; }
    return x;
}

// live instances and unpolled executions of group g: the replica's own (PACK) or the image's (of the same window: the host
// has refused any other)
template <bool PACK>
__device__ __forceinline__ void rspsnap_count(const RspView &v, const RspSnapScal &sc, uint32_t g, uint32_t &ns, uint32_t &nx) {
    ns = rsp_live_n(PACK ? v.len[g] : sc.len[g], v.W);
    nx = PACK ? v.xn[g] : sc.xn[g];
    if (nx > v.W) nx = v.W;                                      // (smr_rsp_exec_poll reads no more)
}

// sums and maxima over the groups [0, g_wave0); g_block0 <= g_wave0 is the same for the whole block
template <bool PACK>
__device__ __forceinline__ void rspsnap_bases(const RspView &v, const RspSnapScal &sc, uint32_t g_block0, uint32_t g_wave0, uint64_t &bs,
                                              uint64_t &bx, uint32_t &ms, uint32_t &mx) {
    __shared__ uint64_t sh_s[4], sh_x[4];
    __shared__ uint32_t sh_ms[4], sh_mx[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t s = 0, x = 0;
    uint32_t xs = 0, xx = 0;
    for (uint32_t g = threadIdx.x; g < g_block0; g += 256) {
        uint32_t ns, nx;
        rspsnap_count<PACK>(v, sc, g, ns, nx);
        s += ns; x += nx; xs = ns > xs ? ns : xs; xx = nx > xx ? nx : xx;
    }
    s = rspsnap_wave_sum(s); x = rspsnap_wave_sum(x); xs = rspsnap_wave_max(xs); xx = rspsnap_wave_max(xx);
    if (lane == 0) { sh_s[w] = s; sh_x[w] = x; sh_ms[w] = xs; sh_mx[w] = xx; }
    __syncthreads();
    bs = sh_s[0] + sh_s[1] + sh_s[2] + sh_s[3];
    bx = sh_x[0] + sh_x[1] + sh_x[2] + sh_x[3];
    ms = sh_ms[0]; mx = sh_mx[0];
    for (int k = 1; k < 4; k++) { ms = sh_ms[k] > ms ? sh_ms[k] : ms; mx = sh_mx[k] > mx ? sh_mx[k] : mx; }
    s = 0; x = 0; xs = 0; xx = 0;
    for (uint32_t g = g_block0 + lane; g < g_wave0; g += 64) {
        uint32_t ns, nx;
        rspsnap_count<PACK>(v, sc, g, ns, nx);
        s += ns; x += nx; xs = ns > xs ? ns : xs; xx = nx > xx ? nx : xx;
    }
    bs += rspsnap_wave_sum(s); bx += rspsnap_wave_sum(x);
    xs = rspsnap_wave_max(xs); xx = rspsnap_wave_max(xx);
    ms = xs > ms ? xs : ms; mx = xx > mx ? xx : mx;
}

__device__ __forceinline__ void rspsnap_zero_pad(uint8_t *base, uint64_t off, uint64_t n) {
    for (uint64_t p = off + n; p < off + rspsnap_a8(n); p++) base[p] = 0;
}

__global__ __launch_bounds__(256) void rsp_snap_pack(const RspSnapArgs A) {
    const RspSnapGeom &Q = A.geo;
    const uint32_t rep = blockIdx.y < SMR_MAX_REPLICAS ? blockIdx.y : 0u;
    const RspView &v = A.v[rep];
    const RspSnapImg S{A.img[rep], A.cap_s[rep], A.cap_x[rep]};
    const RspSnapScal sc = rspsnap_scal(S.base, Q);
    const uint32_t lane = threadIdx.x & 63u, wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t tb0 = blockIdx.x * 4 * Q.tpw, t0 = wv * Q.tpw;
    const uint32_t t1 = t0 + Q.tpw < Q.ntile ? t0 + Q.tpw : Q.ntile;
    const uint32_t gb0 = tb0 * 64 < v.G ? tb0 * 64 : v.G, gw0 = t0 * 64 < v.G ? t0 * 64 : v.G;
    const size_t G = v.G;
    uint64_t bs, bx;
    uint32_t mx_s, mx_x;
    rspsnap_bases<true>(v, sc, gb0, gw0, bs, bx, mx_s, mx_x);
    RspSnapSlot *const recs = (RspSnapSlot *)(S.base + Q.fixed);
    uint32_t *const execs = (uint32_t *)(S.base + rspsnap_off_exec(Q, S));
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t g = t * 64 + lane;
        const bool in = g < v.G;
        uint32_t n = 0, lo = 0, nx = 0;
        if (in) {
            const uint32_t len = v.len[g];
            lo = rsp_live_lo(len, v.W); n = len - lo;
            nx = v.xn[g];
            if (nx > v.W) nx = v.W;
            sc.leader[g] = v.leader[g]; sc.bps[g] = v.bps[g]; sc.bpd[g] = v.bpd[g]; sc.bms[g] = v.bms[g];
            sc.len[g] = len; sc.cbar[g] = v.cbar[g]; sc.ebar[g] = v.ebar[g]; sc.snap[g] = v.snap[g];
            sc.digest[g] = v.digest[g]; sc.xn[g] = nx;
            for (uint32_t p = 0; p < v.R; p++) sc.peb[(size_t)p * G + g] = v.peb[(size_t)p * G + g];
        }
        const uint32_t maxn = rspsnap_wave_max(n), maxx = rspsnap_wave_max(nx);
        mx_s = maxn > mx_s ? maxn : mx_s; mx_x = maxx > mx_x ? maxx : mx_x;
        for (uint32_t k = 0; k < maxn; k++) {
            const bool act = k < n;
            const unsigned long long mask = __ballot(act);
            if (act) {
                const size_t i = (size_t)((lo + k) & v.Wmask) * G + g;
                RspSnapSlot r;
                r.bal = v.s_bal[i]; r.vbal = v.s_vbal[i]; r.pmax = v.s_pmax[i];
                r.val = v.s_val[i]; r.vval = v.s_vval[i]; r.ltrig = v.s_ltrig[i]; r.lendp = v.s_lendp[i]; r.rtrig = v.s_rtrig[i]; r.rendp = v.s_rendp[i];
                r.status = v.s_st[i]; r.mask = v.s_mask[i]; r.vmask = v.s_vmask[i]; r.flags = v.s_fl[i]; r.packs = v.s_packs[i]; r.aacks = v.s_aacks[i];
                r.rsrc = v.s_rsrc[i]; r.zero = 0;
                rsp_slot_canon(r);
                const uint64_t pos = bs + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (pos < S.cap_s) recs[pos] = r;
            }
            bs += (uint64_t)__popcll(mask);
        }
        for (uint32_t j = 0; j < maxx; j++) {
            const bool act = j < nx;
            const unsigned long long mask = __ballot(act);
            if (act) {
                const uint64_t pos = bx + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (pos < S.cap_x) execs[pos] = v.xq[(size_t)j * G + g];
            }
            bx += (uint64_t)__popcll(mask);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {                   // the counters' shards summed (smr_common.h)
        unsigned long long x0 = 0, x1 = 0, x2 = 0, x3 = 0;
        for (uint32_t sh = lane; sh < SMR_CTR_SHARDS; sh += 64) {
            const unsigned long long *c = v.counters + (size_t)sh * SMR_CTR_STRIDE;
            x0 += c[0]; x1 += c[1]; x2 += c[2]; x3 += c[3];
        }
        x0 = rspsnap_wave_sum(x0); x1 = rspsnap_wave_sum(x1); x2 = rspsnap_wave_sum(x2); x3 = rspsnap_wave_sum(x3);
        if (lane == 0) {
            uint64_t *c = (uint64_t *)(S.base + Q.off_ctr);
            c[0] = x0; c[1] = x1; c[2] = x2; c[3] = x3;
        }
    }
    if (t0 < Q.ntile && t1 == Q.ntile && lane == 0) {            // the wavefront of the last tile knows the totals
        RspSnapHdr h;
        h.magic = RSPSNAP_MAGIC; h.version = RSPSNAP_VERSION;
        h.n_groups = v.G; h.population = (uint8_t)v.R; h.me = (uint8_t)v.me; h.fault_tolerance = (uint8_t)v.ft; h.reserved0 = 0;
        h.window = v.W; h.max_live = mx_s;
        h.n_slots = bs; h.n_exec = bx; h.bytes = rspsnap_bytes(Q, bs, bx);
        h.max_exec = mx_x; h.reserved1 = 0; h.reserved2 = 0;
        *(RspSnapHdr *)S.base = h;
        rspsnap_zero_pad(S.base, Q.o_leader, G);                 // padding is zero
        rspsnap_zero_pad(S.base, Q.o_len, 4 * G); rspsnap_zero_pad(S.base, Q.o_cbar, 4 * G); rspsnap_zero_pad(S.base, Q.o_ebar, 4 * G);
        rspsnap_zero_pad(S.base, Q.o_snap, 4 * G); rspsnap_zero_pad(S.base, Q.o_peb, 4 * G * v.R); rspsnap_zero_pad(S.base, Q.o_xn, 4 * G);
        if ((bx & 1) && bx < S.cap_x) execs[bx] = 0;
    }
}

// Load re-establishes: every scalar and peer row, the live instances' ring cells (at slot & Wmask), the unpolled execution
// list, the counters as one shard.  Ring cells outside the live span keep what they held: no handler reads them (RspLane::held,
// ring_lo) and the dump gives null instances there.
__global__ __launch_bounds__(256) void rsp_snap_unpack(const RspSnapArgs A) {
    const RspSnapGeom &Q = A.geo;
    const uint32_t rep = blockIdx.y < SMR_MAX_REPLICAS ? blockIdx.y : 0u;
    const RspView &v = A.v[rep];
    const RspSnapImg S{A.img[rep], A.cap_s[rep], A.cap_x[rep]};
    const RspSnapScal sc = rspsnap_scal(S.base, Q);
    const uint32_t lane = threadIdx.x & 63u, wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t tb0 = blockIdx.x * 4 * Q.tpw, t0 = wv * Q.tpw;
    const uint32_t t1 = t0 + Q.tpw < Q.ntile ? t0 + Q.tpw : Q.ntile;
    const uint32_t gb0 = tb0 * 64 < v.G ? tb0 * 64 : v.G, gw0 = t0 * 64 < v.G ? t0 * 64 : v.G;
    const size_t G = v.G;
    uint64_t bs, bx;
    uint32_t mx_s, mx_x;
    rspsnap_bases<false>(v, sc, gb0, gw0, bs, bx, mx_s, mx_x);
    const RspSnapSlot *const recs = (const RspSnapSlot *)(S.base + Q.fixed);
    const uint32_t *const execs = (const uint32_t *)(S.base + rspsnap_off_exec(Q, S));
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t g = t * 64 + lane;
        const bool in = g < v.G;
        uint32_t n = 0, lo = 0, nx = 0;
        if (in) {
            const uint32_t len = sc.len[g];
            lo = rsp_live_lo(len, v.W); n = len - lo;
            nx = sc.xn[g];
            if (nx > v.W) nx = v.W;                              // (refused by the host: max_exec <= window)
            v.leader[g] = sc.leader[g]; v.bps[g] = sc.bps[g]; v.bpd[g] = sc.bpd[g]; v.bms[g] = sc.bms[g];
            v.len[g] = len; v.cbar[g] = sc.cbar[g]; v.ebar[g] = sc.ebar[g]; v.snap[g] = sc.snap[g];
            v.digest[g] = sc.digest[g]; v.xn[g] = nx;
            for (uint32_t p = 0; p < v.R; p++) v.peb[(size_t)p * G + g] = sc.peb[(size_t)p * G + g];
        }
        const uint32_t maxn = rspsnap_wave_max(n), maxx = rspsnap_wave_max(nx);
        for (uint32_t k = 0; k < maxn; k++) {
            const bool act = k < n;
            const unsigned long long mask = __ballot(act);
            const uint64_t pos = bs + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (act && pos < S.cap_s) {
                const size_t i = (size_t)((lo + k) & v.Wmask) * G + g;
                const RspSnapSlot r = recs[pos];
                v.s_bal[i] = r.bal; v.s_vbal[i] = r.vbal; v.s_pmax[i] = r.pmax;
                v.s_val[i] = r.val; v.s_vval[i] = r.vval; v.s_ltrig[i] = r.ltrig; v.s_lendp[i] = r.lendp; v.s_rtrig[i] = r.rtrig; v.s_rendp[i] = r.rendp;
                v.s_st[i] = r.status; v.s_mask[i] = r.mask; v.s_vmask[i] = r.vmask; v.s_fl[i] = r.flags; v.s_packs[i] = r.packs; v.s_aacks[i] = r.aacks;
                v.s_rsrc[i] = r.rsrc;
            }
            bs += (uint64_t)__popcll(mask);
        }
        for (uint32_t j = 0; j < maxx; j++) {
            const bool act = j < nx;
            const unsigned long long mask = __ballot(act);
            const uint64_t pos = bx + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (act && pos < S.cap_x) v.xq[(size_t)j * G + g] = execs[pos];
            bx += (uint64_t)__popcll(mask);
        }
    }
    static_assert(SMR_CTR_SHARDS == 256, "one thread of block 0 per counter shard");
    if (blockIdx.x == 0)                                         // the sums into shard 0, the other shards zero
        for (uint32_t k = 0; k < SMR_CTR_STRIDE; k++)
            v.counters[(size_t)threadIdx.x * SMR_CTR_STRIDE + k] = (threadIdx.x == 0 && k < 4) ? ((const uint64_t *)(S.base + Q.off_ctr))[k] : 0ull;
}

}  // namespace smr
