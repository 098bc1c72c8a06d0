// A MultiPaxos cluster's state rebuilt from its WAL bytes on the device: WAL bytes -> the canonical image of mp_snapshot.h, which
// smr_mp_load_state / smr_mp_load_groups then place on any ring.
//
// A log is the WAL of one (live replica, group): `[u64 BE length][bincode WalEntry]` frames (server/storage.rs:240-346; mod.rs:261-274:
// PrepareBal 0 { slot, ballot }, AcceptData 1 { slot, ballot, reqs }, CommitSlot 2 { slot }), what smr_wal_prepare_bal / _accept_data /
// _commit_slot write.  The entries are applied in order as MultiPaxosReplica::recover_apply_entry applies them (recovery.rs:10-116,
// release build), starting from what recover_from_snapshot leaves (snapshot.rs:212-216: every bar = start_slot, empty log, ballots 0).
// The engine never sees request bytes: the k-th AcceptData frame of a log takes the k-th token of the log's journal, and of `reqs` only
// the first varint (the Vec's length: empty or not) is read -- the rest is jumped over by the frame's length.
//
// Two walks, one lane per log, no scratch:
//   mp_wal_span    the framing, the statuses, `consumed`, and each log's live span -- the only thing placement needs -- written where
//                  the image keeps it anyway (the scalars start_slot / log_len)
//   mp_wal_apply   snapshot_common.h's tiles and bases over those spans give every SnapSlot its final place; a (tile, replica) unit
//                  zeroes its rows (null instances, packed: snap_place), then each lane walks its log's `consumed` bytes again and
//                  applies the entries into its records, bars and ballots in registers; scalars once at the end, header by the
//                  wavefront of the last tile
// Every read of the WAL buffer is inside the log's own [off, off_next), itself clamped to the buffer.
#pragma once
#include "mp_snapshot.h"
#include "wire_rd.h"

namespace smr {

constexpr uint64_t WAL_MAX_FRAME = 1000000000000ull;     // a length above this is not a frame (safetcp.rs:56-66 says the same of TCP)
enum : uint32_t { WAL_PREPARE_BAL = 0, WAL_ACCEPT_DATA = 1, WAL_COMMIT_SLOT = 2 };

struct WalArgs {
    const uint8_t *__restrict__ buf; uint64_t buf_len;
    const uint64_t *__restrict__ log_off;                   // [n_logs + 1]
    const uint32_t *__restrict__ tok; const uint64_t *__restrict__ tok_off;
    const uint32_t *__restrict__ start;                     // [n_logs] or null: 0
    uint32_t max_span, n_logs;
    uint64_t *__restrict__ consumed; int32_t *__restrict__ status;
    unsigned long long *__restrict__ counts;                // [4], zeroed in front of the first walk
};

// the bytes [p, p + 8) of a log that ends at `end`, little-endian; those at or past `end` read as zero and are never touched
__device__ __forceinline__ uint64_t wal_peek(const uint8_t *__restrict__ buf, uint64_t p, uint64_t end) {
    if (end - p >= 8) return *(const wr_u64_u *)(buf + p);
    uint64_t x = 0;
    for (uint32_t b = 0; p + b < end; b++) x |= (uint64_t)buf[p + b] << (8 * b);
    return x;
}
// one bincode varint at p inside a frame that ends at `fe` (1 / 3 / 5 / 9 bytes); false: it does not parse inside the frame
__device__ __forceinline__ bool wal_varint(const uint8_t *__restrict__ buf, uint64_t &p, uint64_t fe, uint64_t &v) {
    if (p >= fe) return false;
    const uint64_t x = wal_peek(buf, p, fe);
    const uint32_t b = (uint32_t)(x & 0xFF);
    const uint32_t need = b < 251 ? 1 : b == 0xFB ? 3 : b == 0xFC ? 5 : b == 0xFD ? 9 : 0;     // 0xFE (u128), 0xFF: never a usize / u64
    if (need == 0 || fe - p < need) return false;
    v = b;
    if (need == 3) v = (x >> 8) & 0xFFFF;
    else if (need == 5) v = (x >> 8) & 0xFFFFFFFFull;
    else if (need == 9) v = wal_peek(buf, p + 1, fe);
    p += need;
    return true;
}

// one frame of a log
struct WalFrame { uint32_t kind; uint64_t slot, ballot; bool nonempty; uint64_t next; };
enum WalStep { WAL_ENTRY, WAL_END, WAL_CUT, WAL_BAD };
// the frame at p of the log [.., end): WAL_END at the log's end, WAL_CUT where fewer than 8 bytes are left or the length passes the
// end (storage.rs:245-267: read_entry gives None, the final Truncate goes to p), WAL_BAD for a frame that is there and is no WalEntry
__device__ __forceinline__ WalStep wal_frame(const uint8_t *__restrict__ buf, uint64_t p, uint64_t end, WalFrame &f) {
    if (p >= end) return WAL_END;
    if (end - p < 8) return WAL_CUT;
    const uint64_t len = __builtin_bswap64(wal_peek(buf, p, end));
    if (len > WAL_MAX_FRAME) return WAL_BAD;
    if (len > end - p - 8) return WAL_CUT;
    uint64_t q = p + 8;
    const uint64_t fe = q + len;
    uint64_t kind = 0, cnt = 0;
    f.slot = f.ballot = 0; f.nonempty = false; f.next = fe;  // (bytes behind the fields stay unread, as decode_from_slice leaves them)
    if (!wal_varint(buf, q, fe, kind) || kind > WAL_COMMIT_SLOT) return WAL_BAD;
    f.kind = (uint32_t)kind;
    if (!wal_varint(buf, q, fe, f.slot)) return WAL_BAD;
    if (kind != WAL_COMMIT_SLOT && !wal_varint(buf, q, fe, f.ballot)) return WAL_BAD;
    if (kind == WAL_ACCEPT_DATA) {
        if (!wal_varint(buf, q, fe, cnt)) return WAL_BAD;    // ReqBatch = Vec<..>: its length alone
        f.nonempty = cnt != 0;
    }
    return WAL_ENTRY;
}

// log l's bytes, clamped to the buffer (the host has refused descending offsets and offsets past buf_len before the launch)
__device__ __forceinline__ void wal_extent(const WalArgs &A, uint32_t l, uint64_t &lo, uint64_t &hi) {
    lo = A.log_off[l]; hi = A.log_off[l + 1];
    if (lo > A.buf_len) lo = A.buf_len;
    if (hi > A.buf_len) hi = A.buf_len;
    if (hi < lo) hi = lo;
}

// the first walk.  Where a log stops and why depends on the framing, on the journal and on the log's LENGTH as it grows -- not on
// what its instances hold -- so no record is needed yet
__global__ __launch_bounds__(256) void mp_wal_span(const WalArgs A, const SnapImg S) {
    const uint32_t l = blockIdx.x * 256 + threadIdx.x;
    unsigned long long n_applied = 0, n_ignored = 0, n_stopped = 0, n_cut = 0;
    if (l < A.n_logs) {
        uint64_t lo, hi;
        wal_extent(A, l, lo, hi);
        const uint64_t start = A.start ? A.start[l] : 0u;
        const uint64_t t0 = A.tok_off[l], t1 = A.tok_off[l + 1], ntok = t1 > t0 ? t1 - t0 : 0;
        uint64_t p = lo, len = start, k = 0;                 // len = start_slot + insts.len()
        int32_t st = SMR_WAL_ST_OK;
        for (;;) {
            WalFrame f;
            const WalStep w = wal_frame(A.buf, p, hi, f);
            if (w == WAL_END) break;
            if (w == WAL_CUT) { n_cut = 1; break; }
            if (w == WAL_BAD) { st = SMR_WAL_ST_MALFORMED; break; }
            if (f.kind == WAL_ACCEPT_DATA) {                 // every AcceptData frame has a journal entry, applied or not
                if (k >= ntok || (A.tok[t0 + k] != 0) != f.nonempty) { st = SMR_WAL_ST_TOKEN; break; }
                k++;
            }
            if (f.slot < start) { n_ignored++; p = f.next; continue; }          // recovery.rs:16-18, 38-40, 79-81
            if (f.kind == WAL_COMMIT_SLOT) {
                if (f.slot >= len) { st = SMR_WAL_ST_ORDER; break; }            // :84 would index past insts
            } else {
                if (f.slot >= 0xFFFFFFFFull || f.slot - start >= A.max_span) { st = SMR_WAL_ST_RANGE; break; }
                if (f.slot >= len) len = f.slot + 1;                            // :20-22, 42-44
            }
            n_applied++;
            p = f.next;
        }
        A.consumed[l] = p - lo; A.status[l] = st;
        n_stopped = st != SMR_WAL_ST_OK;
        const uint32_t G = S.geo.G, i = l / G, x = l - i * G;
        const SnapScal sc = snap_scal(S.base, S.geo, i);
        sc.start[x] = (uint32_t)start; sc.len[x] = (uint32_t)len; sc.nob[x] = 0;
    }
    n_applied = snap_wave_sum(n_applied); n_ignored = snap_wave_sum(n_ignored); n_stopped = snap_wave_sum(n_stopped); n_cut = snap_wave_sum(n_cut);
    if ((threadIdx.x & 63u) == 0) {
        if (n_applied) atomicAdd(&A.counts[0], n_applied);
        if (n_ignored) atomicAdd(&A.counts[1], n_ignored);
        if (n_stopped) atomicAdd(&A.counts[2], n_stopped);
        if (n_cut) atomicAdd(&A.counts[3], n_cut);
    }
}

// the second walk: one (tile, replica) unit.  base: record index of the unit's first slot on entry, of the next unit's on return.
// sh_n: this wavefront's 64 spans.  Every wavefront of the block calls (block-wide barriers), `live` is false for a tile behind the last
__device__ __forceinline__ void wal_apply_unit(const WalArgs &A, const SnapImg &S, uint32_t i, uint32_t tile, bool live, uint64_t &base, uint32_t &mx,
                                               uint32_t *sh_n) {
    const SnapGeom &Q = S.geo;
    const uint32_t lane = threadIdx.x & 63u, x = tile * 64 + lane;
    const bool in = live && x < Q.G;
    const SnapScal sc = snap_scal(S.base, Q, i);
    const uint32_t start = in ? sc.start[x] : 0u, len = in ? sc.len[x] : 0u;
    uint32_t n = len - start;
    if (n > A.max_span) n = A.max_span;                      // (the first walk has kept every span below it)
    __syncthreads();                                         // the previous unit's readers of sh_n are done
    sh_n[lane] = n;
    __syncthreads();
    SnapSlot *const recs = (SnapSlot *)(S.base + Q.fixed);
    const uint64_t ubase = base;
    // null instances (mod.rs null_instance: ballots 0, Null, empty batch, no bookkeeping) -- a row's records are one contiguous piece,
    // and each lane zeroes its own
    const uint32_t rows = snap_place(n, base, S.cap_slots, lane, [&](uint32_t, uint64_t pos) {
        uint64_t *const w = (uint64_t *)(recs + pos);
#pragma unroll
        for (int j = 0; j < (int)(sizeof(SnapSlot) / 8); j++) w[j] = 0;
    });
    mx = rows > mx ? rows : mx;
    if (!in) return;
    // where row k of this lane went: the rows in front hold min(n_l, k) records of lane l, and row k those of the lanes below with one
    const auto rec = [&](uint32_t k) -> SnapSlot * {
        uint64_t pos = ubase;
        for (uint32_t q = 0; q < 64; q++) { const uint32_t nq = sh_n[q]; pos += nq < k ? nq : k; pos += (q < lane && nq > k) ? 1u : 0u; }
        return pos < S.cap_slots ? recs + pos : nullptr;
    };
    const uint32_t l = i * Q.G + x;
    uint64_t lo, hi;
    wal_extent(A, l, lo, hi);
    const uint64_t took = A.consumed[l];
    if (took < hi - lo) hi = lo + took;                      // only what the first walk accepted
    const uint64_t t0 = A.tok_off[l], t1 = A.tok_off[l + 1], ntok = t1 > t0 ? t1 - t0 : 0;
    uint64_t bps = 0, bpd = 0, bms = 0, p = lo, k = 0;
    uint32_t abar = start, cbar = start, ebar = start;
    for (;;) {
        WalFrame f;
        if (wal_frame(A.buf, p, hi, f) != WAL_ENTRY) break;
        p = f.next;
        uint32_t tok = 0;
        if (f.kind == WAL_ACCEPT_DATA) { tok = k < ntok ? A.tok[t0 + k] : 0u; k++; }
        if (f.slot < start || f.slot - start >= n) continue; // outdated (or what the first walk would have stopped at)
        const uint32_t slot = (uint32_t)f.slot;
        SnapSlot *const c = rec(slot - start);
        if (!c) continue;
        if (f.kind == WAL_PREPARE_BAL) {                     // recovery.rs:24-34
            c->bal = f.ballot; c->status = SMR_ST_PREPARING;
            bps = bps < f.ballot ? f.ballot : bps; bms = bms < f.ballot ? f.ballot : bms;
            bpd = 0;
        } else if (f.kind == WAL_ACCEPT_DATA) {              // :46-75
            c->bal = f.ballot; c->status = SMR_ST_ACCEPTING; c->reqs = tok; c->vbal = f.ballot; c->vreqs = tok;
            bps = bps < f.ballot ? f.ballot : bps; bpd = bpd < f.ballot ? f.ballot : bpd; bms = bms < f.ballot ? f.ballot : bms;
            if (slot == abar) {
                abar++;
                while (abar - start < n) {
                    const SnapSlot *const a = rec(abar - start);
                    if (!a || a->status < SMR_ST_ACCEPTING) break;
                    abar++;
                }
            }
        } else {                                             // :84-111
            c->status = SMR_ST_COMMITTED;
            if (slot == cbar)
                while (cbar < abar) {
                    SnapSlot *const a = rec(cbar - start);
                    if (!a || a->status < SMR_ST_COMMITTED) break;
                    a->status = SMR_ST_EXECUTED;
                    cbar++; ebar++;
                }
        }
    }
    // what recovery leaves of everything else: no leader, no peer's exec_bar, nothing to send
    sc.leader[x] = (uint8_t)NO_REP; sc.bps[x] = bps; sc.bpd[x] = bpd; sc.bms[x] = bms;
    sc.abar[x] = abar; sc.cbar[x] = cbar; sc.ebar[x] = ebar; sc.snap[x] = start; sc.nob[x] = 0;
    for (uint32_t q = 0; q < Q.R; q++) sc.peb[(size_t)q * Q.G + x] = 0;
    if (i == 0) S.base[Q.off_ovf + x] = 0;
}

__global__ __launch_bounds__(256) void mp_wal_apply(const WalArgs A, const SnapImg S) {
    __shared__ uint32_t sh_n[4][64];
    const SnapGeom &Q = S.geo;
    const SnapWave w = snap_wave(Q.tiles, Q.G);
    uint64_t base[1];
    uint32_t mx[1];
    snap_bases<1, 1>([&](uint32_t g, uint64_t (&add)[1], uint32_t (&m)[1]) {
        for (uint32_t i = 0; i < Q.L; i++) {
            const SnapScal sc = snap_scal(S.base, Q, i);
            uint32_t ns = sc.len[g] - sc.start[g];
            if (ns > A.max_span) ns = A.max_span;
            add[0] += ns; m[0] = ns > m[0] ? ns : m[0];
        }
    }, w.gb0, w.gw0, base, mx);
    for (uint32_t j = 0; j < Q.tiles.tpw; j++)               // the same trip count for every wavefront of the launch
        for (uint32_t i = 0; i < Q.L; i++) wal_apply_unit(A, S, i, w.t0 + j, w.t0 + j < w.t1, base[0], mx[0], sh_n[threadIdx.x >> 6]);
    if (blockIdx.x == 0 && threadIdx.x < Q.L) {              // counters 0, no commits on the list
        SnapRep z;
        z.counters[0] = z.counters[1] = z.counters[2] = 0; z.clist_total = z.clist_carried = 0;
        ((SnapRep *)(S.base + Q.off_rep))[threadIdx.x] = z;
    }
    if (w.last && w.lane == 0) {                             // the wavefront of the last tile knows the totals
        SnapHdr h;
        h.magic = SNAP_MAGIC; h.version = SNAP_VERSION;
        h.n_groups = Q.G; h.population = (uint8_t)Q.R; h.commit_extra = (uint8_t)S.commit_extra; h.live_mask = (uint8_t)Q.live; h.reserved0 = 0;
        h.n_slots = base[0]; h.n_outbox = 0; h.n_commits = 0;
        h.bytes = Q.fixed + base[0] * sizeof(SnapSlot);
        h.max_live = mx[0]; h.max_outbox = 0; h.max_commits = 0; h.reserved1 = 0;
        *(SnapHdr *)S.base = h;
        snap_zero_pad(S.base, Q.off_ovf, Q.G);
        for (uint32_t i = 0; i < Q.L; i++) snap_zero_pad(S.base, Q.off_scal + (uint64_t)i * Q.scal_stride, Q.o_leader + Q.G);
    }
}

}  // namespace smr
