// EPaxos command-leader / acceptor hot path over G groups (lane = group), one replica id per
// group: dependency and sequence computation, PreAccept handling, the fast-quorum decision on
// PreAcceptReplies, the slow-path Accept tally and the commit bars.
//
// Stands in for EPaxosReplica::{handle_req_batch (epaxos/request.rs:10-108), first_null_slot
// (mod.rs:485-496), identify_deps / refresh_highest_cols / max_seq_num / DepSet::union
// (dependency.rs:85-167), fast_quorum_eligibility (:175-240), get_enough_identical (:333-367),
// handle_msg_pre_accept (messages.rs:10-93), handle_msg_pre_accept_reply (:96-270),
// handle_msg_accept (:273-345), handle_msg_accept_reply (:348-436),
// handle_logged_{pre_accept,accept,commit}_slot (durability.rs:10-163)}.
// WAL completions are inline (LS-1 rule 0).  A request batch is one Put on one key of a small key
// space, which is all the dependency tracking looks at.
//
// Explicit prepare (smr_ep_cfg.recovery = 1): heartbeat_timeout (heartbeat.rs:17-125: the fast-quorum re-evaluation of
// the PreAccepting instances I lead, ExpPrepare for every in-progress instance of the suspected peer's row, my own
// ExpPrepareReply), handle_msg_exp_prepare (messages.rs:511-574), handle_msg_exp_prepare_reply (:577-821) with
// exp_prepare_next_step (dependency.rs:249-327).  A replica then leads instances outside its own row: the leader
// bookkeeping (PreAcceptReplies held, exp_prepare_voteds) exists for every row, and the handlers take the slot's row apart
// from the message's sender.  Rare, latency-bound work: these kernels are plain lane = group loops over a row's ring.
//
// Dependency-graph execution (execution.rs:25-149 attempt_execution, :152-211 handle_cmd_result,
// durability.rs:136-160) is a separate kernel, ep_execute_kernel, that the entry points launch
// behind their own kernel when smr_ep_cfg.execute is set (see the comment on EpExec).
//
// Layout (group fastest): instance fields X[(row * W + (col & (W-1))) * G + g]; DepSets as R
// consecutive such planes.  The per-key highest columns are the one array indexed by DATA (the command's key, different in
// every group): group-major, hc[(g * n_keys + key) * R + row] -- a lane's R entries are 4 R contiguous bytes of its own
// group's 4 R n_keys, so a wavefront's lookup touches 64-128 lines of 80 KB instead of 5 x (distinct keys) lines, every
// one in a different 256 KB plane (= a different page: the [key][row][G] layout of rounds 1-2).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "smr_common.h"
#include "wire_rd.h"

namespace smr {

constexpr int EMAXR = SMR_MAX_REPLICAS;
constexpr uint32_t EP_NONE = 0xFFFFFFFFu;
constexpr uint8_t EP_NO_KEY = 0xFF;
enum { EST_NULL = 0, EST_PREACCEPTING = 1, EST_ACCEPTING = 2, EST_COMMITTED = 3, EST_EXECUTING = 4, EST_EXECUTED = 5 };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Element `idx` of a device array through a 32-bit BYTE offset (round 4): the engine's arrays are indexed by (row, column,
// group) products that fit 32 bits -- smr_ep_replica_create refuses a geometry whose largest array passes 4 GB -- and an
// address that is "uniform base + 32-bit lane offset" is one global_load with an SGPR base, where the size_t index products
// of rounds 1-3 were 64-bit multiply-adds and add-with-carry chains in front of every access.  The one-launch tick is bound by
// VALU issue (a wave64 VALU instruction occupies its SIMD for four cycles, ~2.5 wavefronts share a SIMD): address arithmetic
// was a fifth of its instructions.
// index arithmetic: a product of two values below 2^24 is ONE full-rate instruction (v_mul_u32_u24 / v_mad_u32_u24) where the
// 32-bit v_mul_lo_u32 is quarter rate -- and the tick kernel has ~400 of them.  smr_ep_replica_create guarantees the operands'
// range (G < 2^24 follows from the 4 GB rule; the reply tables' cell index W * R * R * (recovery ? R : 1) < 2^24 is checked).
#ifdef EP_MUL24
__device__ __forceinline__ uint32_t M24(uint32_t a, uint32_t b) { return __umul24(a, b); }
__device__ __forceinline__ uint32_t SHL_OF(uint32_t x, uint32_t pow2) { return x << (uint32_t)__builtin_ctz(pow2); }
#else
__device__ __forceinline__ uint32_t M24(uint32_t a, uint32_t b) { return a * b; }
__device__ __forceinline__ uint32_t SHL_OF(uint32_t x, uint32_t pow2) { return x * pow2; }
#endif
template <typename T>
__device__ __forceinline__ T &EA(T *base, uint32_t idx) { return *(T *)((char *)base + (uint32_t)(idx * (uint32_t)sizeof(T))); }

// An instance is ONE RECORD of 16-byte words, each word a plane [R][W][G] (group fastest, so a wavefront's access to a word is
// one contiguous 1 KB request):
//   p0 = { bal lo, bal hi, seq lo, seq hi }
//   p1 = { deps[0..3] }
//   p2 = { deps[4], m0, m1, deps[5] }     m0 = status | key << 8 | bk << 16 | pa_acks << 24   (bk: has_lbk | has_rbk << 1 | source << 2)
//                                          m1 = acc_acks | avoid_fast_path << 8 | exp_prepare_acks << 16 | exp_prepare has-entry bits << 24
//   p3 = { deps[6], deps[7], -, - }        (populations 7 and 8 only)
// Rounds 1-2 kept every field in a plane of its own: a handler that takes an instance was 13 loads or 13 stores of 1-8 bytes.
// The one-launch tick's time turned out to be its NUMBER of memory instructions (profiles/round3/r3o: ~0.65 us per load or store,
// whatever its width), so the fields a handler touches together now travel together: an instance is 3 loads or 3 stores.
struct EpView {
    uint32_t G, W, Wmask, R, me, n_keys, simple_q, super_q;
    uint32_t hc_ew;                      // words of an hc entry: 8 at R <= 6 (32 bytes, four keys to a cache line), else 16
    uint32_t hc_es, hc_kv;               // words between the entries of two keys (= hc_ew; round 5: 32 where a cluster shares one table --
                                         //     smr_ep_cluster_create: the R replicas' entries of a (group, key) in ONE 128-byte line);
                                         //     the word of an entry that holds the executor's KV word
    u32x4 *p0, *p1, *p2, *p3;            // [R][W][G] each; p3 NULL at populations <= 6
    uint32_t *sq32;                      // [R][W][G] round 6: min(seq, 2^32 - 1) of every cell, kept beside p0 by every store of it -- max_seq_num
                                         //     (dependency.rs:101-109) looks at R sequence numbers per PreAccept and nothing else of those cells:
                                         //     4 bytes per lane instead of a 16-byte word (25 such loads per lane and tick, 0.3 of 2.8 KB); a cell
                                         //     that reads 2^32 - 1 sends its reader to p0
    uint64_t *pa_seq;                    // my row only: [W][R][G]
    uint32_t *pa_deps;                   // my row only: [W][R][R][G]
    uint32_t *len, *commit_bars;         // [R][G]
    uint32_t *my_nulls;                  // [G] null instances currently in my own row (first_null_slot need not scan at 0)
    uint8_t *rewritten;                  // [G] sticky: a message once rewrote a cell below its row's commit bar (a duplicate, a late or an explicit-prepare
                                         //     message): from then on "below the exec bar" no longer means Executed for this group (EpExecLaneT::attempt)
    uint32_t *hc;                        // [G][n_keys][hc_ew]: per (group, key) the key's highest column in each row (words 0 .. R) and, round 4, the
                                         //     executor's KV word of the key (the last two words): both are lines of the lane's own -- a gather and a
                                         //     scatter each -- and an instance's PreAccept touches the first a phase or two before its execution touches
                                         //     the second; in one line, the second is a cache hit more often than not
    unsigned long long *counters;        // fast commits, slow-path entries, slow-path commits; explicit prepare outcomes:
                                         // Committed, Accepting, PreAccepting with a command, PreAccepting as a no-op
    // explicit prepare (recovery != 0; pa_seq / pa_deps then hold every row: [R][W][R][G] / [R][W][R][R][G])
    uint32_t recovery;
    uint64_t *xp_max;                    // [R][W][G] exp_prepare_max_bal (avoid_fast_path, exp_prepare_acks and the has-entry bits: m1)
    uint8_t *xv_status, *xv_key;         // [R][W][R][G] exp_prepare_voteds
    uint64_t *xv_seq;
    uint32_t *xv_deps;                   // [R][W][R][R][G]
};

// an instance in registers
template <int NR>
struct EpInst {
    uint64_t bal, seq;
    uint32_t d[NR];
    uint32_t m0, m1;
    __device__ __forceinline__ uint32_t status() const { return m0 & 0xFFu; }
    __device__ __forceinline__ uint32_t key() const { return (m0 >> 8) & 0xFFu; }
    __device__ __forceinline__ uint32_t bk() const { return (m0 >> 16) & 0xFFu; }
    __device__ __forceinline__ uint32_t pa_acks() const { return m0 >> 24; }
    __device__ __forceinline__ uint32_t acc_acks() const { return m1 & 0xFFu; }
    __device__ __forceinline__ uint32_t avoid() const { return (m1 >> 8) & 0xFFu; }
    __device__ __forceinline__ uint32_t xp_acks() const { return (m1 >> 16) & 0xFFu; }
    __device__ __forceinline__ uint32_t xp_has() const { return m1 >> 24; }
    __device__ __forceinline__ void set_status(uint32_t x) { m0 = (m0 & ~0xFFu) | (x & 0xFFu); }
    __device__ __forceinline__ void set_key(uint32_t x) { m0 = (m0 & ~0xFF00u) | ((x & 0xFFu) << 8); }
    __device__ __forceinline__ void set_bk(uint32_t x) { m0 = (m0 & ~0xFF0000u) | ((x & 0xFFu) << 16); }
    __device__ __forceinline__ void set_pa_acks(uint32_t x) { m0 = (m0 & 0x00FFFFFFu) | (x << 24); }
    __device__ __forceinline__ void set_acc_acks(uint32_t x) { m1 = (m1 & ~0xFFu) | (x & 0xFFu); }
    __device__ __forceinline__ void set_avoid(uint32_t x) { m1 = (m1 & ~0xFF00u) | ((x & 0xFFu) << 8); }
    __device__ __forceinline__ void set_xp_acks(uint32_t x) { m1 = (m1 & ~0xFF0000u) | ((x & 0xFFu) << 16); }
    __device__ __forceinline__ void set_xp_has(uint32_t x) { m1 = (m1 & 0x00FFFFFFu) | (x << 24); }
    __device__ __forceinline__ void make_null() {                            // mod.rs:467-480
        bal = 0; seq = 0; m0 = (uint32_t)EP_NO_KEY << 8; m1 = 0;
#pragma unroll
        for (int k = 0; k < NR; k++) d[k] = EP_NONE;
    }
};

// CACHE: the lane keeps its group's per-row scalars (row lengths, commit bars, my_nulls) in registers from load_scalars() to
// store_scalars() -- the one-launch cluster tick runs ~15 handlers on a lane, and every one of them starts with these
// words; a handler kernel of its own (CACHE = false) reads and writes them in place
// CACHE: the lane keeps its group's per-row scalars (row lengths, commit bars; the executor's exec bars and commit-bar copies)
// from load_scalars() to store_scalars() in a block of LDS the kernel hands it (bind_cache: [4][NR][64] words per wavefront,
// word = [array][row][lane]) -- the one-launch cluster tick runs ~15 handlers on a lane, and every one of them starts with these
// words; a handler kernel of its own (CACHE = false) reads and writes them in place.  (Round 3 kept them in 21 registers, every
// access a chain of NR compare-and-selects because `row` is a run-time value: since round 4 an access is one ds_read / ds_write,
// and the registers went to the handlers.)
#if defined(__HIP_DEVICE_COMPILE__)
#define SMR_L __attribute__((address_space(3)))
#else
#define SMR_L
#endif
#ifdef EPC_STAMPS
#define EPC_SUB(L, k) do { __builtin_amdgcn_s_waitcnt(0); if ((L).sub) (L).sub[k] = wall_clock64(); } while (0)   /* experiments only */
#else
#define EPC_SUB(L, k) do { } while (0)
#endif

template <int NR, bool CACHE = false>
struct EpLaneT {
#ifdef EPC_STAMPS
    unsigned long long *sub = nullptr;   // experiments only: where this lane writes the sub-stamps of one handler (tools/dbg_epc_stamps.py)
#endif
    const EpView &v;
    const uint32_t g;
    unsigned int n_fast = 0, n_slow = 0, n_acc = 0, n_xc = 0, n_xa = 0, n_xp = 0, n_xn = 0;
    SMR_L uint32_t *lc = nullptr;                                            // CACHE: this lane's column of the wavefront's cache block
    uint32_t c_nulls = 0;
    bool rewritten = false;                                                  // CACHE: v.rewritten[g]
    // a handler is about to rewrite the existing cell (row, col), possibly to a lower Status
    __device__ __forceinline__ void note_rewrite(uint32_t col, uint32_t cb_of_row) {
        if (col < cb_of_row) { rewritten = true; EA(v.rewritten, g) = 1; }
    }
    __device__ __forceinline__ EpLaneT(const EpView &v_, uint32_t g_) : v(v_), g(g_) {}
    __device__ __forceinline__ void bind_cache(uint32_t *block_of_my_wavefront, uint32_t lane) { lc = (SMR_L uint32_t *)(block_of_my_wavefront + lane); }
    __device__ __forceinline__ SMR_L uint32_t &cw(int arr, uint32_t row) const { return lc[((uint32_t)arr * NR + row) * 64u]; }
    __device__ __forceinline__ void load_scalars() {
        if (!CACHE) return;
        for (uint32_t r = 0; r < v.R; r++) { cw(0, r) = EA(v.len, M24(r, v.G) + g); cw(1, r) = EA(v.commit_bars, M24(r, v.G) + g); }
        c_nulls = EA(v.my_nulls, g);
        rewritten = EA(v.rewritten, g) != 0;
    }
    __device__ __forceinline__ void store_scalars() const {
        if (!CACHE) return;
        for (uint32_t r = 0; r < v.R; r++) { EA(v.len, M24(r, v.G) + g) = cw(0, r); EA(v.commit_bars, M24(r, v.G) + g) = cw(1, r); }
        EA(v.my_nulls, g) = c_nulls;
    }
    __device__ __forceinline__ uint32_t get_len(uint32_t row) const { return CACHE ? cw(0, row) : EA(v.len, M24(row, v.G) + g); }
    __device__ __forceinline__ void set_len(uint32_t row, uint32_t x) { if (CACHE) cw(0, row) = x; else EA(v.len, M24(row, v.G) + g) = x; }
    __device__ __forceinline__ uint32_t get_cb(uint32_t row) const { return CACHE ? cw(1, row) : EA(v.commit_bars, M24(row, v.G) + g); }
    __device__ __forceinline__ void set_cb(uint32_t row, uint32_t x) { if (CACHE) cw(1, row) = x; else EA(v.commit_bars, M24(row, v.G) + g) = x; }
    __device__ __forceinline__ uint32_t get_nulls() const { return CACHE ? c_nulls : EA(v.my_nulls, g); }
    __device__ __forceinline__ void add_nulls(uint32_t d) { if (CACHE) c_nulls += d; else EA(v.my_nulls, g) += d; }
    // the plane of the reply tables a (row, col) instance uses: one per row with recovery, else my row's only
    __device__ __forceinline__ uint32_t pw(uint32_t row, uint32_t col) const { return M24(v.recovery ? row : 0u, v.W) + (col & v.Wmask); }
    __device__ __forceinline__ uint32_t ps_ix(uint32_t row, uint32_t col, uint32_t peer) const { return M24(M24(pw(row, col), v.R) + peer, v.G) + g; }
    __device__ __forceinline__ uint32_t pd_ix(uint32_t row, uint32_t col, uint32_t peer, uint32_t k) const {
        return M24(M24(M24(pw(row, col), v.R) + peer, v.R) + k, v.G) + g;
    }
    __device__ __forceinline__ uint32_t xv_ix(uint32_t row, uint32_t col, uint32_t peer) const {
        return M24(M24(M24(row, v.W) + (col & v.Wmask), v.R) + peer, v.G) + g;
    }
    // ---- the instance record (see EpView) ----
    __device__ __forceinline__ uint32_t ix(uint32_t row, uint32_t col) const { return M24(M24(row, v.W) + (col & v.Wmask), v.G) + g; }
    __device__ __forceinline__ static void unpack_p2(u32x4 w, EpInst<NR> &I) {
        if (NR > 4) I.d[4 < NR ? 4 : 0] = w.x;
        I.m0 = w.y; I.m1 = w.z;
        if (NR > 5) I.d[5 < NR ? 5 : 0] = w.w;
    }
    __device__ __forceinline__ static u32x4 pack_p2(const EpInst<NR> &I) {
        return (u32x4){NR > 4 ? I.d[4 < NR ? 4 : 0] : EP_NONE, I.m0, I.m1, NR > 5 ? I.d[5 < NR ? 5 : 0] : EP_NONE};
    }
    __device__ __forceinline__ EpInst<NR> load_inst(uint32_t i) const {        // every word of the record in one round of loads
        EpInst<NR> I;
        const u32x4 a = EA(v.p0, i), b = EA(v.p1, i), c = EA(v.p2, i);
        I.bal = (uint64_t)a.x | ((uint64_t)a.y << 32); I.seq = (uint64_t)a.z | ((uint64_t)a.w << 32);
#pragma unroll
        for (int k = 0; k < NR; k++) I.d[k] = EP_NONE;
        I.d[0] = b.x;
        if (NR > 1) I.d[1 < NR ? 1 : 0] = b.y;
        if (NR > 2) I.d[2 < NR ? 2 : 0] = b.z;
        if (NR > 3) I.d[3 < NR ? 3 : 0] = b.w;
        unpack_p2(c, I);
        if (NR > 6 && v.R > 6) { const u32x4 e = EA(v.p3, i); I.d[6 < NR ? 6 : 0] = e.x; I.d[7 < NR ? 7 : 0] = e.y; }
        return I;
    }
    __device__ __forceinline__ void store_p0(uint32_t i, const EpInst<NR> &I) const {
        EA(v.p0, i) = (u32x4){(uint32_t)I.bal, (uint32_t)(I.bal >> 32), (uint32_t)I.seq, (uint32_t)(I.seq >> 32)};
        EA(v.sq32, i) = I.seq < 0xFFFFFFFFull ? (uint32_t)I.seq : 0xFFFFFFFFu;
    }
    __device__ __forceinline__ void store_deps(uint32_t i, const EpInst<NR> &I) const {   // p1, p2 (with the meta words) and p3
        EA(v.p1, i) = (u32x4){I.d[0], NR > 1 ? I.d[1 < NR ? 1 : 0] : EP_NONE, NR > 2 ? I.d[2 < NR ? 2 : 0] : EP_NONE, NR > 3 ? I.d[3 < NR ? 3 : 0] : EP_NONE};
        EA(v.p2, i) = pack_p2(I);
        if (NR > 6 && v.R > 6) EA(v.p3, i) = (u32x4){I.d[6 < NR ? 6 : 0], I.d[7 < NR ? 7 : 0], 0u, 0u};
    }
    __device__ __forceinline__ void store_inst(uint32_t i, const EpInst<NR> &I) const { store_p0(i, I); store_deps(i, I); }
    // the words that hold Status / key / bookkeeping / ack masks (and deps[4], deps[5]): a read-modify-write of ONE word of the record
    __device__ __forceinline__ void load_meta(uint32_t i, EpInst<NR> &I) const { unpack_p2(EA(v.p2, i), I); }
    __device__ __forceinline__ void store_meta(uint32_t i, const EpInst<NR> &I) const { EA(v.p2, i) = pack_p2(I); }
    __device__ __forceinline__ uint32_t status_at(uint32_t i) const { return EA(v.p2, i).y & 0xFFu; }
    __device__ __forceinline__ uint64_t seq_at(uint32_t i) const {
        const uint32_t s = EA(v.sq32, i);
        if (s != 0xFFFFFFFFu) return s;
        const u32x4 a = EA(v.p0, i);
        return (uint64_t)a.z | ((uint64_t)a.w << 32);
    }
    __device__ __forceinline__ uint64_t bal_at(uint32_t i) const { const u32x4 a = EA(v.p0, i); return (uint64_t)a.x | ((uint64_t)a.y << 32); }
    __device__ __forceinline__ void fresh_leader_bk(uint32_t i, EpInst<NR> &I) const {   // request.rs:48-57, heartbeat.rs:88-97
        I.set_bk(I.bk() | 1u);
        I.set_pa_acks(0); I.set_acc_acks(0);
        if (v.recovery) { I.set_xp_acks(0); I.set_xp_has(0); EA(v.xp_max, i) = 0; }
    }
    // is the column still in the row's ring of W instances (the harness guard)
    __device__ __forceinline__ bool held(uint32_t row, uint32_t col) const {
        const uint32_t end = get_len(row);
        return col < end && col + v.W >= end;
    }
    // `write` = false: the caller is about to store the whole record of that very cell itself
    __device__ __forceinline__ void push_null(uint32_t row, bool write = true) {            // mod.rs:467-480
        const uint32_t col = get_len(row);
        if (write) {
            EpInst<NR> I;
            I.make_null();
            store_inst(ix(row, col), I);
        }
        set_len(row, col + 1);
        if (row == v.me) add_nulls(1u);
    }
    __device__ __forceinline__ void identify_deps(uint32_t key, uint32_t (&d)[NR]) const {   // dependency.rs:113-137
#pragma unroll
        for (int i = 0; i < NR; i++) d[i] = (key != EP_NO_KEY && (uint32_t)i < v.R) ? EA(v.hc, SHL_OF(M24(g, v.n_keys) + key, v.hc_es) + i) : EP_NONE;
    }
    __device__ __forceinline__ uint64_t max_seq_num(const uint32_t (&d)[NR]) const {         // dependency.rs:101-109
        uint64_t m = 0;
#pragma unroll
        for (int row = 0; row < NR; row++) {
            if ((uint32_t)row >= v.R || d[row] == EP_NONE || !held(row, d[row])) continue;
            const uint64_t s = seq_at(ix(row, d[row]));
            if (s > m) m = s;
        }
        return m;
    }
    __device__ __forceinline__ void refresh_highest_cols(uint32_t row, uint32_t col, uint32_t key) {   // dependency.rs:141-167
        if (key == EP_NO_KEY) return;
        const uint32_t o = SHL_OF(M24(g, v.n_keys) + key, v.hc_es) + row;
        const uint32_t hc = EA(v.hc, o);
        if (hc == EP_NONE || col > hc) EA(v.hc, o) = col;
    }
    // `known` (optional): the meta words of the cell (row, col) as the caller just stored them -- the walk starts at that very
    // cell, and re-reading what was written an instant ago is a round trip to memory on the handler's critical path
    __device__ __forceinline__ void logged_commit_slot(uint32_t row, uint32_t col, const EpInst<NR> *known = nullptr) {   // durability.rs:104-135
        uint32_t cb = get_cb(row);
        if (col != cb) return;
        while (cb < get_len(row) && held(row, cb)) {
            const uint32_t i = ix(row, cb);
            EpInst<NR> I;
            if (known && cb == col) { I.m0 = known->m0; I.m1 = known->m1; I.d[NR > 4 ? 4 : 0] = known->d[NR > 4 ? 4 : 0]; if (NR > 5) I.d[NR > 5 ? 5 : 0] = known->d[NR > 5 ? 5 : 0]; }
            else load_meta(i, I);
            if (I.status() < EST_COMMITTED) break;
            if (I.key() == EP_NO_KEY) { I.set_status(EST_EXECUTED); store_meta(i, I); }
            cb++;
        }
        set_cb(row, cb);
    }
    // messages.rs:348-436 on an instance I lead
    __device__ __forceinline__ void accept_reply(uint32_t peer, uint32_t row, uint32_t col, uint64_t ballot) {
        if (!held(row, col)) return;
        const uint32_t i = ix(row, col);
        EpInst<NR> I;
        load_meta(i, I);
        if (I.status() != EST_ACCEPTING || !(I.bk() & 1) || bal_at(i) != ballot) return;   // :371-376
        uint32_t acks = I.acc_acks();
        if ((acks >> peer) & 1u) return;
        acks |= 1u << peer;
        I.set_acc_acks(acks);
        const bool commit = (uint32_t)__popc(acks) >= v.simple_q;                // :386
        if (commit) I.set_status(EST_COMMITTED);
        store_meta(i, I);
        if (commit) {
            n_acc++;
            logged_commit_slot(row, col);
        }
    }
    // messages.rs:96-270 on an instance I lead; rd = the reply's DepSet
    __device__ __forceinline__ void pre_accept_reply(uint32_t peer, uint32_t row, uint32_t col, uint64_t ballot, uint64_t rseq,
                                                     const uint32_t (&rd)[NR], uint32_t exploded) {
        const uint32_t R = v.R;
        if (!held(row, col)) return;                                             // :125-127
        const uint32_t i = ix(row, col);
        EpInst<NR> I = load_inst(i);
        if (I.status() != EST_PREACCEPTING || (ballot > 0 && I.bal != ballot) || !(I.bk() & 1)) return;   // :129-134
        uint32_t acks = I.pa_acks();
        if ((acks >> peer) & 1u) return;                                         // :136-138
        if (ballot > 0) {                                                        // :141-144
            EA(v.pa_seq, ps_ix(row, col, peer)) = rseq;
            for (uint32_t k = 0; k < R; k++) EA(v.pa_deps, pd_ix(row, col, peer, k)) = rd[k];
            acks |= 1u << peer;
            I.set_pa_acks(acks);
            store_meta(i, I);
        }
        const bool avoid = v.recovery && I.avoid();                              // dependency.rs:196
        // dependency.rs:175-240 fast_quorum_eligibility
        const uint32_t all_cnt = __popc(acks);
        if (all_cnt < v.simple_q) return;
        // the replies held, in registers: seq + DepSet of every acked peer
        uint64_t ps[NR]; uint32_t pd[NR][NR];
#pragma unroll
        for (int p = 0; p < NR; p++) {
            const bool on = (uint32_t)p < R && ((acks >> p) & 1u);
            ps[p] = on ? EA(v.pa_seq, ps_ix(row, col, p)) : 0;
#pragma unroll
            for (int k = 0; k < NR; k++)
                pd[p][k] = (on && (uint32_t)k < R) ? EA(v.pa_deps, pd_ix(row, col, p, k)) : EP_NONE;
        }
        // dependency.rs:333-367 get_enough_identical: size of the largest class of equal (seq, deps)
        uint32_t max_cnt = 0; int best = -1;
#pragma unroll
        for (int p = 0; p < NR; p++) {
            if (!((acks >> p) & 1u) || (uint32_t)p >= R) continue;
            uint32_t same = 0;
#pragma unroll
            for (int q = 0; q < NR; q++) {
                if (!((acks >> q) & 1u) || (uint32_t)q >= R) continue;
                bool eq = ps[q] == ps[p];
#pragma unroll
                for (int k = 0; k < NR; k++) eq = eq && pd[q][k] == pd[p][k];
                same += eq ? 1u : 0u;
            }
            if (same > max_cnt) { max_cnt = same; best = p; }
        }
        uint32_t bad = 0;
#pragma unroll
        for (int p = 0; p < NR; p++)
            if ((uint32_t)p < R && !((acks >> p) & 1u) && (uint32_t)p != v.me && ((exploded >> p) & 1u)) bad++;
        uint64_t dseq = 0; uint32_t dd[NR];
        int next = 0;
        if (!avoid && max_cnt >= v.super_q) {                                    // fast path
            next = EST_COMMITTED;
            dseq = 0;
#pragma unroll
            for (int p = 0; p < NR; p++) if (p == best) dseq = ps[p];
#pragma unroll
            for (int k = 0; k < NR; k++) {
                dd[k] = EP_NONE;
#pragma unroll
                for (int p = 0; p < NR; p++) if (p == best) dd[k] = pd[p][k];
            }
        } else if (avoid || max_cnt + (R - bad - all_cnt) < v.super_q) {         // :221-236 slow path: union / max
            next = EST_ACCEPTING;
#pragma unroll
            for (int k = 0; k < NR; k++) dd[k] = EP_NONE;
#pragma unroll
            for (int p = 0; p < NR; p++) {
                if (!((acks >> p) & 1u) || (uint32_t)p >= R) continue;
                if (ps[p] > dseq) dseq = ps[p];
#pragma unroll
                for (int k = 0; k < NR; k++) {                                // dependency.rs:85-97 union
                    if (dd[k] != EP_NONE) { if (pd[p][k] != EP_NONE && pd[p][k] > dd[k]) dd[k] = pd[p][k]; }
                    else dd[k] = pd[p][k];
                }
            }
        }
        if (next == 0) return;
        I.seq = dseq;
#pragma unroll
        for (int k = 0; k < NR; k++) I.d[k] = (uint32_t)k < R ? dd[k] : EP_NONE;
        I.set_status(next == EST_COMMITTED ? EST_COMMITTED : EST_ACCEPTING);
        store_inst(i, I);
        if (next == EST_COMMITTED) {                                             // :158-206
            n_fast++;
            logged_commit_slot(row, col);
        } else {                                                                 // :209-262
            n_slow++;
            accept_reply(v.me, row, col, I.bal);                                 // durability.rs:78-83
        }
    }
    // messages.rs:577-821 with exp_prepare_next_step (dependency.rs:249-327) and the WAL completions of what it logs;
    // returns the Status of the message it broadcasts for (row, col) under new_ballot (the instance holds its seq / deps /
    // reqs), 0 = none
    __device__ __forceinline__ int exp_prepare_reply(uint32_t peer, uint32_t row, uint32_t col, uint64_t nb, uint64_t vbal,
                                                     uint32_t vstatus, uint64_t vseq, const uint32_t (&vd)[NR], uint32_t vkey) {
        const uint32_t R = v.R;
        if (!held(row, col)) return 0;                                           // :599-601
        const uint32_t i = ix(row, col);
        EpInst<NR> I = load_inst(i);
        if (nb <= I.bal || !(I.bk() & 1)) return 0;                              // :603-605
        uint32_t acks = I.xp_acks(), has = I.xp_has();
        if ((acks >> peer) & 1u) return 0;                                       // :607-609
        uint64_t mx = EA(v.xp_max, i);
        if (vbal > mx) { has = 0; mx = vbal; EA(v.xp_max, i) = mx; }                 // :612-615
        if (vbal >= mx) {                                                        // :616-621
            has |= 1u << peer;
            const uint32_t q = xv_ix(row, col, peer);
            EA(v.xv_status, q) = (uint8_t)vstatus; EA(v.xv_seq, q) = vseq; EA(v.xv_key, q) = (uint8_t)vkey;
            for (uint32_t k = 0; k < R; k++) EA(v.xv_deps, (q / v.G * R + k) * v.G + g) = vd[k];
        }
        acks |= 1u << peer;
        I.set_xp_acks(acks); I.set_xp_has(has);
        store_meta(i, I);
        if ((uint32_t)__popc(acks) < v.simple_q) return 0;                       // dependency.rs:257-260
        // the voted entries, in registers
        uint32_t xs[NR], xk[NR]; uint64_t xq[NR]; uint32_t xd[NR][NR];
#pragma unroll
        for (int p = 0; p < NR; p++) {
            const bool on = (uint32_t)p < R && ((has >> p) & 1u);
            const uint32_t q = xv_ix(row, col, on ? p : 0);
            xs[p] = on ? EA(v.xv_status, q) : 0xFFu; xq[p] = on ? EA(v.xv_seq, q) : 0; xk[p] = on ? EA(v.xv_key, q) : EP_NO_KEY;
#pragma unroll
            for (int k = 0; k < NR; k++) xd[p][k] = (on && (uint32_t)k < R) ? EA(v.xv_deps, (q / v.G * R + k) * v.G + g) : EP_NONE;
        }
        int has_commit = -1, has_accept = -1, has_pre = -1;                      // :264-273: the highest peer id of a status
#pragma unroll
        for (int p = 0; p < NR; p++) {
            if (xs[p] == EST_COMMITTED) has_commit = p;
            else if (xs[p] == EST_ACCEPTING) has_accept = p;
            else if (xs[p] == EST_PREACCEPTING) has_pre = p;
        }
        int next = 0, pick = -1;
        if (has_commit >= 0) { next = EST_COMMITTED; pick = has_commit; }
        else if (has_accept >= 0) { next = EST_ACCEPTING; pick = has_accept; }
        else {
            if (mx == (uint64_t)(row + 1)) {                                     // :286-311 make_default_ballot(slot_row)
                uint32_t n = 0;
#pragma unroll
                for (int p = 0; p < NR; p++) n += ((uint32_t)p != row && xs[p] == EST_PREACCEPTING) ? 1u : 0u;
                if (n + 1 >= v.simple_q && n > 0) {
#pragma unroll
                    for (int p = 0; p < NR; p++) {                            // a class of >= simple_q equal entries: at most one
                        if ((uint32_t)p == row || xs[p] != EST_PREACCEPTING || pick >= 0) continue;
                        uint32_t same = 0;
#pragma unroll
                        for (int q = 0; q < NR; q++) {
                            bool eq = (uint32_t)q != row && xs[q] == EST_PREACCEPTING && xq[q] == xq[p] && xk[q] == xk[p];
#pragma unroll
                            for (int k = 0; k < NR; k++) eq = eq && xd[q][k] == xd[p][k];
                            same += eq ? 1u : 0u;
                        }
                        if (same >= v.simple_q) { next = EST_ACCEPTING; pick = p; }
                    }
                }
            }
            if (!next) { next = EST_PREACCEPTING; pick = has_pre; }              // :316-327 (pick < 0: the no-op)
        }
        uint64_t dseq = 1; uint32_t dkey = EP_NO_KEY; uint32_t dd[NR];
#pragma unroll
        for (int k = 0; k < NR; k++) dd[k] = EP_NONE;
#pragma unroll
        for (int p = 0; p < NR; p++)
            if (p == pick) {
                dseq = xq[p]; dkey = xk[p];
#pragma unroll
                for (int k = 0; k < NR; k++) dd[k] = xd[p][k];
            }
        note_rewrite(col, get_cb(row));
        I.bal = nb; I.set_status((uint32_t)next); I.seq = dseq; I.set_key(dkey);
#pragma unroll
        for (int k = 0; k < NR; k++) I.d[k] = (uint32_t)k < R ? dd[k] : EP_NONE;
        if (next == EST_PREACCEPTING) I.set_avoid(1);                            // :747-815
        store_inst(i, I);
        refresh_highest_cols(row, col, dkey);
        if (next == EST_COMMITTED) { n_xc++; logged_commit_slot(row, col); }     // :637-690
        else if (next == EST_ACCEPTING) { n_xa++; accept_reply(v.me, row, col, nb); }   // :692-745
        else {
            if (dkey == EP_NO_KEY) n_xn++; else n_xp++;
            pre_accept_reply(v.me, row, col, nb, dseq, dd, 0u);
        }
        return next;
    }
    __device__ __forceinline__ void flush() {
        unsigned int c[7] = {n_fast, n_slow, n_acc, n_xc, n_xa, n_xp, n_xn};
        for (int k = 0; k < (v.recovery ? 7 : 3); k++) {
            unsigned int x = c[k];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
            if (__lane_id() == 0 && x) ctr_add(v.counters, k, (unsigned long long)x);
        }
    }
};
typedef EpLaneT<EMAXR, false> EpLane;

// ---- dependency-graph execution ------------------------------------------------------------------
// One call of a handler kernel moves at most one row's commit bar per group (one message or one
// instance per group per call), so the attempts the reference makes inside handle_logged_commit_slot
// (durability.rs:136-160) can run right behind the handler: ep_execute_kernel finds the row whose
// commit bar differs from the copy it kept (prev_cb) and does, for tail = (row, commit_bar - 1):
//   attempt_execution(tail); if it ran: the re-attempts on every row whose tail is still Committed;
//   then the results of the submitted commands in submission order (LS-1 rule 0).
// What attempt_execution builds (execution.rs:33-83): a breadth-first walk over deps + the implicit
// row predecessor; a NEW node gets one edge, from the slot popped just before it (:57-59), and
// GraphMap::add_edge inserts that slot as a node if it is not one (a pruned, already executing slot
// then runs again).  Every node has at most one incoming edge, made when it joins, so the graph is
// a forest, every strongly connected component is a single node (the oracle runs the full Tarjan
// and counts the exceptions: none) and tarjan_scc's output (:87-93) is the depth-first post-order:
// trees started from nodes in insertion order, children newest edge first.  The per-component sort
// by seq (:99-102) has nothing to sort.
// The walk needs no queue: pops are the tail followed by the pushes of each new node in the order
// the nodes joined.  Per group: nodes in insertion order (nslot, bit 15 = new), the forest as
// head / sib / parent links over node ids, node_of[ring cell] = node id + 1, and the submissions of
// the whole call in `order`; all uint16 [index][G].
// the executor's KV word in 32 bits: a token is (row + 1) << 32 | col with row + 1 <= 8, and the word keeps 28 bits of the column.  A
// column grows by at most one per tick: 2^28 ticks are 3.1 days at 1 kHz and 6.5 hours at the 0.09 ms ticks of the bench (ADVICE
// r5: round 5's comment said years).  An instance executed at a column >= 2^28 would leave a word that unpacks to another
// token: the executor COUNTS such submissions (EpExecLaneT::c_kvovf, counter slot 3) and smr_ep_exec_dump / smr_ep_exec_poll
// answer SMR_ERR_STATE from then on instead of handing out tokens that are not the reference's.
constexpr uint32_t EP_KV_COL_LIMIT = 1u << 28;
__host__ __device__ __forceinline__ uint32_t ep_kv_pack(uint64_t tok) { return tok ? (uint32_t)((tok >> 32) << 28) | ((uint32_t)tok & 0x0FFFFFFFu) : 0u; }
__host__ __device__ __forceinline__ uint64_t ep_kv_unpack(uint32_t w) { return w ? ((uint64_t)(w >> 28) << 32) | (w & 0x0FFFFFFFu) : 0ull; }
constexpr uint16_t XNIL = 0xFFFF;
constexpr uint16_t XNEW = 0x8000;
constexpr uint64_t EP_DG_MUL = 0x100000001B3ull;

struct EpExec {
    uint32_t *exec_bars, *prev_cb;       // [R][G]
                                         // (the KV words -- token of the last Put, 0 = none -- live in the hc entries: EpView::hc)
    uint64_t *digest;                    // [G] chain over (token, old token) in submission order
    uint16_t *node_of, *nslot, *head, *sib, *parent;   // [R*W][G]
    uint16_t *order;                     // [2*R*W][G] this call's submissions (ring cells), ...
    uint32_t *n_sub;                     // ... [G] how many: what smr_ep_exec_poll reads
    unsigned long long *counters;        // commands submitted, re-submissions, pops of an instance no longer held,
                                         // (unused: components > 1 node), attempts, abandoned attempts
};

}  // namespace smr
#include "ep_snapshot.h"   // save / load of a replica's state: the canonical image, its two kernels, the live-span rule the dumps share
namespace smr {

template <int NR, bool CACHE = false>
struct EpExecLaneT {
    const EpView &v;
    const EpExec &x;
    EpLaneT<NR, CACHE> &L;
    // CACHE: exec_bars / prev_cb in arrays 2 and 3 of the lane's LDS cache block (see EpLaneT)
    __device__ __forceinline__ void load_scalars() {
        if (!CACHE) return;
        for (uint32_t r = 0; r < v.R; r++) { L.cw(2, r) = EA(x.exec_bars, M24(r, v.G) + g); L.cw(3, r) = EA(x.prev_cb, M24(r, v.G) + g); }
    }
    __device__ __forceinline__ void store_scalars() const {
        if (!CACHE) return;
        for (uint32_t r = 0; r < v.R; r++) { EA(x.exec_bars, M24(r, v.G) + g) = L.cw(2, r); EA(x.prev_cb, M24(r, v.G) + g) = L.cw(3, r); }
    }
    __device__ __forceinline__ uint32_t get_eb(uint32_t row) const { return CACHE ? L.cw(2, row) : EA(x.exec_bars, M24(row, v.G) + g); }
    __device__ __forceinline__ void set_eb(uint32_t row, uint32_t y) { if (CACHE) L.cw(2, row) = y; else EA(x.exec_bars, M24(row, v.G) + g) = y; }
    // every row's exec bar in one round of loads (CACHE: they are in LDS and nothing is loaded here), and one of them
    // (known_executed_below: 0 for every row of a group in which a cell below a commit bar was once rewritten --
    // EpView::rewritten: there a cell below the exec bar may have been taken back to an earlier Status, and the walk must look)
    __device__ __forceinline__ void load_ebs(uint32_t (&ebs)[NR]) {
        if (!CACHE) L.rewritten = EA(v.rewritten, g) != 0;
#pragma unroll
        for (int q = 0; q < NR; q++) ebs[q] = (!CACHE && (uint32_t)q < v.R) ? EA(x.exec_bars, (uint32_t)M24(q, v.G) + g) : 0u;
    }
    __device__ __forceinline__ uint32_t known_executed_below(const uint32_t (&ebs)[NR], uint32_t row) const {
        return L.rewritten ? 0u : eb_of(ebs, row);
    }
    __device__ __forceinline__ uint32_t eb_of(const uint32_t (&ebs)[NR], uint32_t row) const {
        if (CACHE) return L.cw(2, row);
        uint32_t y = 0;
#pragma unroll
        for (int q = 0; q < NR; q++) if ((uint32_t)q == row) y = ebs[q];
        return y;
    }
    // has the row's commit bar moved since the last look (then the copy follows it)
    __device__ __forceinline__ bool cb_moved(uint32_t row, uint32_t cb) {
        if (!CACHE) {
            const uint32_t o = M24(row, v.G) + g;
            if (cb == EA(x.prev_cb, o)) return false;
            EA(x.prev_cb, o) = cb;
            return true;
        }
        if (L.cw(3, row) == cb) return false;
        L.cw(3, row) = cb;
        return true;
    }
    const uint32_t g, wshift;
    uint32_t n_nodes = 0, n_order = 0, last = XNIL;          // last: ring cell of the slot popped before, XNIL = none / not held
    uint32_t last_node = 0;                                  // node_of[last] (node id + 1; 0: not a node), kept beside it
    bool reins = false;                                      // this attempt made a node of an executed cell (add_edge's missing endpoint)
    unsigned int c_exec = 0, c_reexec = 0, c_unheld = 0, c_attempts = 0, c_aborts = 0;
    unsigned int c_kvovf = 0;                                // submissions whose column does not fit the 32-bit KV word (ep_kv_pack)
    __device__ __forceinline__ EpExecLaneT(const EpView &v_, const EpExec &x_, EpLaneT<NR, CACHE> &L_, uint32_t g_)
        : v(v_), x(x_), L(L_), g(g_), wshift(31u - (uint32_t)__clz((int)v_.W)) {}
    // (the walk's arrays are [index][G] planes of the arena -- or, where the caller hands the lane private ones (walk_in: a few lanes of a
    // kernel that has LDS to spare, ep_cluster_commit_one_by_one_kernel), [index][stride] with the lane's column `off`: every access of
    // the walk is a dependent round trip, ~30 of them per attempt with a second node)
    uint32_t at_stride = 0, at_off = 0;
    __device__ __forceinline__ void walk_in(uint32_t stride, uint32_t off) { at_stride = stride; at_off = off; }
    __device__ __forceinline__ uint32_t at(uint32_t i) const { return at_stride ? i * at_stride + at_off : M24(i, v.G) + g; }
    // the KV word of a key: word hc_kv of the key's hc entry (EpView::hc) -- the token of the key's last Put, (row + 1) << 32 | col,
    // packed into 32 bits (ep_kv_pack: 4 bits of row + 1, 28 of the column; 0 = none) so that five replicas' entries fit one line
    __device__ __forceinline__ uint32_t &kv_at(uint32_t key) const { return EA(v.hc, SHL_OF(M24(g, v.n_keys) + key, v.hc_es) + v.hc_kv); }
    // the column a ring cell of this row holds (the one of its residue among the last W)
    __device__ __forceinline__ uint32_t col_of(uint32_t row, uint32_t w) const {
        const uint32_t end = L.get_len(row), lo = end > v.W ? end - v.W : 0u;
        uint32_t c = (lo & ~v.Wmask) | w;
        if (c < lo) c += v.W;
        return c;
    }
    __device__ __forceinline__ uint32_t new_node(uint32_t ring, uint16_t flag) {
        const uint32_t id = n_nodes++;
        EA(x.nslot, at(id)) = (uint16_t)(ring | flag);
        EA(x.head, at(id)) = XNIL; EA(x.sib, at(id)) = XNIL; EA(x.parent, at(id)) = XNIL;
        EA(x.node_of, at(ring)) = (uint16_t)(id + 1);
        return id;
    }
    // One pop of the walk (execution.rs:37-82) behind its commit-bar and ring checks, on a cell whose Status `st` and node_of
    // word `no` the caller has at hand.  A node made here changes node_of[ring] and -- add_edge's missing endpoint --
    // possibly node_of[last]: (p1, v1) / (p2, v2) = (ring cell, its new node_of word) for the caller to patch the copies it
    // holds, XNONE = no such change.  node_of[last] itself is tracked in last_node, so an edge costs no load.
    static constexpr uint32_t XNONE = 0xFFFFFFFFu, XUNUSED = 0xFFFFFFFEu;
    __device__ __forceinline__ void visit(uint32_t ring, uint32_t st, uint32_t no, uint32_t &p1, uint32_t &v1, uint32_t &p2, uint32_t &v2) {
        p1 = p2 = XNONE; v1 = v2 = 0;
        if (st >= EST_EXECUTING || no != 0) { last = ring; last_node = no; return; }   // :46-54
        const uint32_t id = new_node(ring, XNEW);                                // :56-59
        p1 = ring; v1 = id + 1;
        if (last != XNIL) {
            uint32_t a = last_node;
            if (a == 0) { a = new_node(last, 0) + 1; c_reexec++; reins = true; p2 = last; v2 = a; }   // add_edge inserts the missing endpoint
            a -= 1;
            EA(x.sib, at(id)) = EA(x.head, at(a)); EA(x.head, at(a)) = (uint16_t)id; EA(x.parent, at(id)) = (uint16_t)a;
        }
        last = ring; last_node = id + 1;
    }
    // execution.rs:105-142 for one node's instance, sync_exec = false
    __device__ __forceinline__ void submit_ring(uint32_t ring) {
        const uint32_t row = ring >> wshift, col = col_of(row, ring & v.Wmask);
        const uint32_t i = L.ix(row, col);
        EpInst<NR> I;
        L.load_meta(i, I);
        const uint32_t key = I.key();
        if (key != EP_NO_KEY) {
            const uint64_t tok = ((uint64_t)(row + 1) << 32) | col, old = ep_kv_unpack(kv_at(key));
            if (col >= EP_KV_COL_LIMIT) c_kvovf++;
            kv_at(key) = ep_kv_pack(tok);
            uint64_t d = EA(x.digest, g);
            d = (d ^ tok) * EP_DG_MUL; d = (d ^ old) * EP_DG_MUL;
            EA(x.digest, g) = d;
            if (n_order < 2u * v.R * v.W) EA(x.order, at(n_order++)) = (uint16_t)ring;   // (the list's capacity; beyond it a result would not come: never seen)
            c_exec++;
        }
        I.set_status(EST_EXECUTING);
        L.store_meta(i, I);
    }
    // attempt_execution (execution.rs:25-149) from the tail (trow, tcol).  The walk is latency, not bytes: a lane's loads are
    // round trips to HBM one behind the other, so a node's R dependencies and its row predecessor are looked at with all
    // their words loaded up front (deps; then Status + node_of of the R + 1 cells), not cell by cell -- the pops still happen
    // one by one, in the reference's order, on those copies (patched where an earlier pop of the batch made a node).
    __device__ __forceinline__ bool attempt(uint32_t trow, uint32_t tcol) {
        c_attempts++;
        n_nodes = 0; last = XNIL; last_node = 0; reins = false;
        bool abandoned = false;
        uint32_t p1, v1, p2, v2, ring0 = XNIL;
        uint32_t ebs[NR];
        load_ebs(ebs);                                                           // (no exec bar moves inside an attempt)
        if (tcol >= L.get_cb(trow)) abandoned = true;                            // :41-45
        else if (!L.held(trow, tcol)) { c_unheld++; last = XNIL; }               // harness: left the ring = executed
        else {
            ring0 = (trow << wshift) | (tcol & v.Wmask);
            const uint32_t st = L.status_at(L.ix(trow, tcol)), no = EA(x.node_of, at(ring0));
            visit(ring0, st, no, p1, v1, p2, v2);
        }
        for (uint32_t i = 0; !abandoned && i < n_nodes; i++) {
            const uint32_t s = (i == 0) ? (ring0 | XNEW) : EA(x.nslot, at(i));      // (node 0 is the tail, new by construction)
            if (!(s & XNEW)) continue;
            const uint32_t ring = s & 0x7FFFu, row = ring >> wshift, col = col_of(row, ring & v.Wmask);
            uint32_t cc[NR + 1], cr[NR + 1], cst[NR + 1], cno[NR + 1];           // per cell: column, ring cell (XUNUSED: no pop), Status, node_of
            {
                const EpInst<NR> I = L.load_inst(L.ix(row, col));                // :62-73 its dependencies, row order
#pragma unroll
                for (int k = 0; k < NR; k++) cc[k] = (uint32_t)k < v.R ? I.d[k] : EP_NONE;
            }
            cc[NR] = col > 0 ? col - 1 : EP_NONE;                                // :74-77 the row predecessor
#pragma unroll
            for (int e = 0; e <= NR; e++) {
                const uint32_t erow = e < NR ? (uint32_t)e : row;
                const bool on = cc[e] != EP_NONE;
                const uint32_t r_ = on ? erow : 0u, c_ = on ? cc[e] : 0u, rg = (r_ << wshift) | (c_ & v.Wmask);
                cr[e] = on ? rg : XUNUSED;
                // a cell below its row's exec bar is Executed, and no node unless this attempt made it one (node_of is zero
                // outside an attempt; inside, an executed cell becomes a node only as add_edge's missing endpoint -- `reins`;
                // one made in this very batch is patched in below): nothing to load -- and that is most dependencies and every
                // row predecessor of a cluster that keeps up.  (These are gathers: a lane's cell is a cache line of its own.)
                // (no branch around a load -- the join would wait for it: a lane that needs nothing loads cell (0, 0), which every
                // such lane of the device shares, and drops the word)
                const bool need = on && c_ >= known_executed_below(ebs, r_), need_no = need || (on && reins);
                cst[e] = L.status_at(L.ix(need ? r_ : 0u, need ? c_ : 0u));
                cno[e] = EA(x.node_of, at(need_no ? rg : 0u));
                if (!need) cst[e] = EST_EXECUTED;
                if (!need_no) cno[e] = 0u;
            }
#pragma unroll
            for (int e = 0; e <= NR; e++) {
                if (abandoned || cr[e] == XUNUSED) continue;
                const uint32_t erow = e < NR ? (uint32_t)e : row;
                if (cc[e] >= L.get_cb(erow)) { abandoned = true; continue; }     // :41-45
                if (!L.held(erow, cc[e])) { c_unheld++; last = XNIL; continue; }
                visit(cr[e], cst[e], cno[e], p1, v1, p2, v2);
#pragma unroll
                for (int f = e + 1; f <= NR; f++) {
                    if (cr[f] == p1) cno[f] = v1;
                    if (cr[f] == p2) cno[f] = v2;
                }
            }
        }
        if (abandoned) {
            c_aborts++;
            for (uint32_t i = 0; i < n_nodes; i++) EA(x.node_of, at(EA(x.nslot, at(i)) & 0x7FFFu)) = 0;
            return false;
        }
        if (n_nodes == 1) {                                                      // the tail alone (no edge was made): no links to walk
            EA(x.node_of, at(ring0)) = 0;
            submit_ring(ring0);
            return true;
        }
        // post-order over the forest; entering a node clears its node_of cell (= visited, and the cleanup)
        for (uint32_t root = 0; root < n_nodes; root++) {
            const uint32_t rr = EA(x.nslot, at(root)) & 0x7FFFu;
            if (EA(x.node_of, at(rr)) == 0) continue;
            EA(x.node_of, at(rr)) = 0;
            uint32_t u = root;
            for (;;) {
                const uint32_t c = EA(x.head, at(u));
                if (c != XNIL) {
                    EA(x.head, at(u)) = EA(x.sib, at(c));
                    const uint32_t cr_ = EA(x.nslot, at(c)) & 0x7FFFu;
                    if (EA(x.node_of, at(cr_)) != 0) { EA(x.node_of, at(cr_)) = 0; u = c; }
                } else {
                    submit_ring(EA(x.nslot, at(u)) & 0x7FFFu);
                    if (u == root) break;
                    u = EA(x.parent, at(u));
                }
            }
        }
        return true;
    }
    // execution.rs:152-211, one command per instance
    __device__ __forceinline__ void cmd_result(uint32_t ring) {
        const uint32_t row = ring >> wshift, col = col_of(row, ring & v.Wmask);
        {
            const uint32_t i = L.ix(row, col);
            EpInst<NR> I;
            L.load_meta(i, I);
            I.set_status(EST_EXECUTED);
            L.store_meta(i, I);
        }
        uint32_t eb = get_eb(row);
        if (col != eb) return;
        eb++;                                                                    // (col itself: Executed just now)
        while (eb < L.get_len(row) && L.held(row, eb) && L.status_at(L.ix(row, eb)) >= EST_EXECUTED) eb++;
        set_eb(row, eb);
    }
    // durability.rs:136-160 for the row whose commit bar moved
    // (APPEND: a handler that runs several of the reference's inner handlers in one call -- heartbeat_timeout -- keeps the
    // call's earlier submissions in `order`; each inner handler's results still come right behind it)
    template <bool APPEND = false>
    __device__ __forceinline__ void advanced(uint32_t row, uint32_t cb) {
        if (!APPEND) n_order = 0;
        const uint32_t first = n_order;
        if (attempt(row, cb - 1)) {
            uint32_t re = 0;                                                     // rows to re-attempt, found before any of them runs
#pragma unroll
            for (int q = 0; q < NR; q++) {                                       // (the R tails' Status words: one round of loads)
                const uint32_t qq = (uint32_t)q < v.R ? (uint32_t)q : 0u, c = L.get_cb(qq);
                const bool ok = (uint32_t)q < v.R && c > get_eb(qq) && L.held(qq, c - 1);
                const uint32_t st = L.status_at(L.ix(qq, ok ? c - 1 : 0u));
                if (ok && st == EST_COMMITTED) re |= 1u << q;
            }
            for (uint32_t q = 0; q < v.R; q++)
                if ((re >> q) & 1u) (void)attempt(q, L.get_cb(q) - 1);
        }
        for (uint32_t i = first; i < n_order; i++) cmd_result(EA(x.order, at(i)));
    }
    // `advanced` for the common case behind a handler that has the committed instance in registers: the row's commit bar went
    // from the instance's column to the next (tail = that instance, H = its record as stored, a real command), and every cell
    // the walk pops from it -- its dependencies, its row predecessor -- turns out executed or gone: a single-node graph.
    // Then nothing of the walk needs memory but the popped cells' Status words, and those, the R rows' tails for the
    // re-attempt scan, the cell behind mine for the exec-bar scan and the KV / digest words all go out in ONE round of loads
    // (node_of is zero everywhere between attempts, so a first pop never needs it).  Returns false -- having touched nothing
    // -- when the case is another one; `advanced` then does it in general.
    __device__ __forceinline__ bool advanced_hinted(uint32_t row, uint32_t cb, const EpInst<NR> &H, uint32_t hcol) {
        const uint32_t key = H.key();
        if (hcol + 1 != cb || H.status() != EST_COMMITTED || key == EP_NO_KEY || !L.held(row, hcol)) return false;
        const uint32_t R = v.R;
        uint32_t ebs[NR];
        load_ebs(ebs);
        uint32_t cc[NR + 1], cst[NR + 1];
#pragma unroll
        for (int k = 0; k < NR; k++) cc[k] = (uint32_t)k < R ? H.d[k] : EP_NONE;
        cc[NR] = hcol > 0 ? hcol - 1 : EP_NONE;
#pragma unroll
        for (int e = 0; e <= NR; e++) {
            const uint32_t erow = e < NR ? (uint32_t)e : row;
            const bool need = cc[e] != EP_NONE && cc[e] >= known_executed_below(ebs, erow);         // below the exec bar: Executed (see attempt)
            cst[e] = L.status_at(L.ix(need ? erow : 0u, need ? cc[e] : 0u));     // (no branch around a load: see attempt)
            if (!need) cst[e] = EST_EXECUTED;
        }
        uint32_t tst[NR]; bool tok[NR];
#pragma unroll
        for (int q = 0; q < NR; q++) {
            const uint32_t qq = (uint32_t)q < R ? (uint32_t)q : 0u, c = L.get_cb(qq);
            tok[q] = (uint32_t)q < R && c > eb_of(ebs, qq) && L.held(qq, c - 1);
            tst[q] = L.status_at(L.ix(qq, tok[q] ? c - 1 : 0u));
        }
        // (the cell behind mine matters to the exec-bar scan only: when the bar is at my column and that cell exists)
        const bool need_n = hcol == eb_of(ebs, row) && hcol + 1 < L.get_len(row) && L.held(row, hcol + 1);
        const uint32_t nst = L.status_at(L.ix(row, need_n ? hcol + 1 : 0u));
        const uint64_t old = ep_kv_unpack(kv_at(key));
        uint64_t dg = EA(x.digest, g);
        EPC_SUB(L, 10);
        // the pops, in the reference's order, on those words
        bool abandoned = false;
        uint32_t unheld = 0;
#pragma unroll
        for (int e = 0; e <= NR; e++) {
            if (abandoned || cc[e] == EP_NONE) continue;
            const uint32_t erow = e < NR ? (uint32_t)e : row;
            if (cc[e] >= L.get_cb(erow)) { abandoned = true; continue; }         // :41-45
            if (!L.held(erow, cc[e])) { unheld++; continue; }
            if (cst[e] < EST_EXECUTING) return false;                            // a second node: the general walk
        }
        c_attempts++; c_unheld += unheld;
        if (abandoned) { c_aborts++; return true; }                              // (nothing was stored, nothing to clean up)
        // the graph is the tail alone: submit it (execution.rs:105-142)
        const uint32_t i = L.ix(row, hcol);
        const uint32_t ring = (row << wshift) | (hcol & v.Wmask);
        EpInst<NR> I = H;
        const uint32_t first = n_order;
        {
            const uint64_t tok_ = ((uint64_t)(row + 1) << 32) | hcol;
            if (hcol >= EP_KV_COL_LIMIT) c_kvovf++;
            kv_at(key) = ep_kv_pack(tok_);
            dg = (dg ^ tok_) * EP_DG_MUL; dg = (dg ^ old) * EP_DG_MUL;
            EA(x.digest, g) = dg;
            if (n_order < 2u * v.R * v.W) EA(x.order, at(n_order++)) = (uint16_t)ring;
            c_exec++;
        }
        uint32_t re = 0;                                                         // rows to re-attempt (my own tail is Executing now)
#pragma unroll
        for (int q = 0; q < NR; q++)
            if (tok[q] && (uint32_t)q != row && tst[q] == EST_COMMITTED) re |= 1u << q;
        if (re) {                                                                // rare: the general walk for those, results in order
            I.set_status(EST_EXECUTING);
            L.store_meta(i, I);
            for (uint32_t q = 0; q < R; q++)
                if ((re >> q) & 1u) (void)attempt(q, L.get_cb(q) - 1);
            for (uint32_t k = first; k < n_order; k++) cmd_result(EA(x.order, at(k)));
            return true;
        }
        if (n_order > first) {                                                   // my command's result (execution.rs:152-211)
            I.set_status(EST_EXECUTED);
            L.store_meta(i, I);
            uint32_t eb = get_eb(row);
            if (hcol == eb) {
                eb++;
                if (eb < L.get_len(row) && L.held(row, eb) && nst >= EST_EXECUTED) {
                    eb++;
                    while (eb < L.get_len(row) && L.held(row, eb) && L.status_at(L.ix(row, eb)) >= EST_EXECUTED) eb++;
                }
                set_eb(row, eb);
            }
        } else {                                                                 // (the order list was full: no result comes)
            I.set_status(EST_EXECUTING);
            L.store_meta(i, I);
        }
        return true;
    }
    // the attempts of handle_logged_commit_slot for whichever row's commit bar the inner handler just moved (at most one)
    __device__ __forceinline__ void after_inner_handler() {
        for (uint32_t row = 0; row < v.R; row++) {
            const uint32_t cb = L.get_cb(row);
            if (!cb_moved(row, cb)) continue;
            advanced<true>(row, cb);
        }
    }
    __device__ __forceinline__ void flush() {
        unsigned int c[6] = {c_exec, c_reexec, c_unheld, c_attempts, c_aborts, c_kvovf};
        const int slot[6] = {0, 1, 2, 4, 5, 3};
        for (int k = 0; k < 6; k++) {
            unsigned int y = c[k];
            for (int off = 32; off > 0; off >>= 1) y += __shfl_xor(y, off);
            if (__lane_id() == 0 && y) ctr_add(x.counters, (int)slot[k], (unsigned long long)y);
        }
    }
};
typedef EpExecLaneT<EMAXR, false> EpExecLane;

// ---- the handlers on one lane (= one group of one replica): what the per-handler kernels below and the one-kernel
// cluster tick (ep_cluster_tick_kernel) both run ---------------------------------------------------------------------------
// the attempts of handle_logged_commit_slot behind ONE handler (durability.rs:136-160): at most one row's commit bar moved
// (hint: the instance (hrow, hcol) the handler committed, as it stored it -- see advanced_hinted)
template <int NR, bool C>
__device__ __forceinline__ void ep_exec_after_handler(const EpView &v, const EpExec &x, EpExecLaneT<NR, C> &E, const EpInst<NR> *hint = nullptr,
                                                      uint32_t hrow = 0, uint32_t hcol = 0) {
    E.n_order = 0;
    for (uint32_t row = 0; row < v.R; row++) {
        const uint32_t cb = E.L.get_cb(row);
        if (!E.cb_moved(row, cb)) continue;
        if (hint && row == hrow && E.advanced_hinted(row, cb, *hint, hcol)) { EPC_SUB(E.L, 11); continue; }
        EPC_SUB(E.L, 12);
        E.advanced(row, cb);
        EPC_SUB(E.L, 13);
    }
    EA(x.n_sub, E.g) = E.n_order;                                                // 0 when no commit bar moved
}

// request.rs:10-108 + my own PreAcceptSlot completion (durability.rs:25-35): key k (EP_NO_KEY: nothing to propose);
// (of, oc, os, d) = the PreAccept to broadcast
template <int NR, bool C>
__device__ __forceinline__ void ep_propose_lane(EpLaneT<NR, C> &L, uint32_t k, uint32_t ex, uint8_t &of, uint32_t &oc, uint64_t &os,
                                                uint32_t (&d)[NR], bool *hc_later = nullptr, bool *rec_later = nullptr) {
    // hc_later: the key's entry is the caller's to update.  rec_later: where the instance takes a fresh cell at the row's end, neither its
    // record nor my own PreAcceptReply is stored -- *rec_later = true, and both are the caller's (ep_cluster_tick_pm_kernel: materialize_own)
    const EpView &v = L.v;
    of = 0; oc = 0; os = 0;
#pragma unroll
    for (int i = 0; i < NR; i++) d[i] = EP_NONE;
    if (k == EP_NO_KEY) return;
    const uint32_t row = v.me;
    uint32_t col = EP_NONE;                                                  // mod.rs:485-496 (exec_bars stay 0 here)
    const uint32_t end = L.get_len(row);
    EpInst<NR> I;
    I.make_null();
    if (L.get_nulls() != 0)                                                  // only a PreAccept / Accept for my own row pads it
        for (uint32_t c = end > v.W ? end - v.W : 0; c < end; c++) {
            EpInst<NR> J;
            L.load_meta(L.ix(row, c), J);
            if (J.status() == EST_NULL) { col = c; I.m0 = J.m0; I.m1 = J.m1; break; }   // (a padded slot may carry replica bookkeeping: explicit prepare)
        }
    const bool at_end = col == EP_NONE;
    if (col == EP_NONE) { L.push_null(row, false); col = L.get_len(row) - 1; }   // (the null record itself is never stored: the whole cell is, below)
    L.add_nulls(0xFFFFFFFFu);                                                      // the slot stops being null
    L.identify_deps(k, d);                                                   // (one round: the key's R highest columns)
    uint64_t seq = 0;
    {                                                                        // max_seq_num: the R sequence numbers in one round
        bool ok[NR]; uint64_t sq[NR];
#pragma unroll
        for (int q = 0; q < NR; q++) {
            ok[q] = (uint32_t)q < v.R && d[q] != EP_NONE && L.held((uint32_t)q < v.R ? q : 0, d[q]);
            sq[q] = L.seq_at(L.ix((uint32_t)q < v.R ? q : 0, ok[q] ? d[q] : 0u));
        }
#pragma unroll
        for (int q = 0; q < NR; q++) if (ok[q] && sq[q] > seq) seq = sq[q];
        seq += 1;
    }
    const uint32_t i = L.ix(row, col);
    const uint64_t bal = (uint64_t)(v.me + 1);                               // make_default_ballot
    I.bal = bal; I.seq = seq; I.set_key(k);
#pragma unroll
    for (int q = 0; q < NR; q++) I.d[q] = (uint32_t)q < v.R ? d[q] : EP_NONE;
    {                                                                        // refresh_highest_cols: hc[key][row] is d[row], loaded above
        uint32_t hc_row = EP_NONE;
#pragma unroll
        for (int q = 0; q < NR; q++) if ((uint32_t)q == row) hc_row = d[q];
        const bool up = hc_row == EP_NONE || col > hc_row;
        if (hc_later) *hc_later = up;
        else if (up) EA(v.hc, SHL_OF(M24(L.g, v.n_keys) + k, v.hc_es) + row) = col;
    }
    L.fresh_leader_bk(i, I);
    I.set_status(EST_PREACCEPTING);
    I.set_pa_acks(1u << v.me);                                               // (my own PreAcceptReply, below)
    of = 1; oc = col; os = seq;
    if (rec_later && at_end && !v.recovery) { *rec_later = true; return; }
    L.store_inst(i, I);
    // my own PreAcceptReply (durability.rs:25-35 -> messages.rs:96-270) on bookkeeping that is fresh: it is recorded and is the
    // only one held, and one reply is below any quorum (simple_q >= 2 at populations >= 3) -- handle_msg_pre_accept_reply
    // returns at dependency.rs:205 without looking at `ex`
    EA(v.pa_seq, L.ps_ix(row, col, v.me)) = seq;
    for (uint32_t q = 0; q < v.R; q++) {
        uint32_t x = EP_NONE;
#pragma unroll
        for (int qq = 0; qq < NR; qq++) if ((uint32_t)qq == q) x = d[qq];
        EA(v.pa_deps, L.pd_ix(row, col, v.me, q)) = x;
    }
    (void)ex;
}

// messages.rs:10-93 (MODE 0: PreAccept) / :273-345 (MODE 1: Accept) / :438-508 (MODE 2: CommitNotice) + the acceptor's
// WAL completion, for the message (src, row, c, b, s, deps[i * G + g], k) if `on`; (of, ob, os, d) = the reply
// LBK = false: the caller knows the instance cannot carry leader bookkeeping at this replica (another replica's row in a
// cluster without explicit prepare), and the branch that answers the leader's own message is left out
// (ep_acceptor_lane_in: the message's DepSet already in registers -- the one-launch tick takes it out of LDS)
template <int MODE, int NR, bool LBK, bool C>
__device__ __forceinline__ void ep_acceptor_lane_in(EpLaneT<NR, C> &L, bool on, uint32_t src, uint32_t row, uint32_t c, uint64_t b, uint64_t s,
                                                    uint32_t (&in)[NR], uint32_t k, uint8_t &of, uint64_t &ob, uint64_t &os,
                                                    uint32_t (&d)[NR], EpInst<NR> *rec = nullptr, bool *stored = nullptr) {
    const EpView &v = L.v;
    const uint32_t g = L.g;
    of = 0; ob = 0; os = 0;
    if (stored) *stored = false;
#pragma unroll
    for (int i = 0; i < NR; i++) d[i] = EP_NONE;
    // The handler is a chain of memory round trips and little else, so its loads are issued in as few ROUNDS as the data
    // dependences allow, unconditionally and from clamped (always valid) addresses -- what a round loads for a message that
    // turns out not to be taken is dropped:
    //   round 1 (with the caller's loads of the message's scalars): the message's DepSet
    //   round 2: the cell's ballot and meta words, the key's highest columns
    //   round 3 (PreAccept): the sequence numbers of the key's highest instances
    const uint32_t rw = row < v.R ? row : 0u;
    const uint32_t i = L.ix(rw, c);
    const bool need_meta = LBK || MODE != 0 || rw == v.me;                   // (LBK = false: Status / bookkeeping are read only where they can matter;
    const u32x4 w0 = EA(v.p0, i);                                            //  a CommitNotice leaves the bookkeeping as it is)
    u32x4 w2 = (u32x4){EP_NONE, (uint32_t)EP_NO_KEY << 8, 0u, EP_NONE};
    if (need_meta) w2 = EA(v.p2, i);
    const uint32_t kk = k != EP_NO_KEY ? k : 0u;
    uint32_t my[NR];
#pragma unroll
    for (int q = 0; q < NR; q++)
        my[q] = (MODE == 0 && (uint32_t)q < v.R) ? EA(v.hc, SHL_OF(M24(g, v.n_keys) + kk, v.hc_es) + q) : EP_NONE;
    EPC_SUB(L, 1);
    if (!on) return;
    if (!(row < v.R && !(c < L.get_len(row) && !L.held(row, c)))) return;    // col < start_col analogue
    // :33-36 pad the row up to the column; the cell of the column itself is written below if the message is taken (a fresh
    // cell's ballot is 0: it always is), so its null record is not stored first
    bool fresh = false;
    while (L.get_len(row) <= c) { fresh = L.get_len(row) == c; L.push_null(row, !fresh); }
    EPC_SUB(L, 2);
    EpInst<NR> I;
    I.make_null();
    if (!fresh) {
        I.bal = (uint64_t)w0.x | ((uint64_t)w0.y << 32);
        if (need_meta) L.unpack_p2(w2, I);
    }
    if (!(b >= I.bal)) return;                                               // :40
    if (row == v.me && I.status() == EST_NULL) L.add_nulls(0xFFFFFFFFu);
    uint32_t hc_row = EP_NONE;                                               // hc[key][row] as loaded: refresh_highest_cols needs no second look
#pragma unroll
    for (int q = 0; q < NR; q++) if ((uint32_t)q == row) hc_row = my[q];
    // An Accept / CommitNotice for a cell that already holds an instance of this key (its PreAccept came by here): the key's
    // highest column in this row was raised to at least c when that instance was stored and never falls, so
    // refresh_highest_cols has nothing to do -- and hc[g][key] is a cache line of this lane's own, not fetched.  Otherwise
    // (the PreAccept was lost) the word is loaded now, one round trip later than the rest.
    const bool hc_known = MODE != 0 && !fresh && I.status() != EST_NULL && I.key() == k;
    if (MODE != 0 && !hc_known && k != EP_NO_KEY) hc_row = EA(v.hc, SHL_OF(M24(g, v.n_keys) + k, v.hc_es) + row);
    if (MODE == 0) {
        if (k == EP_NO_KEY) {
#pragma unroll
            for (int q = 0; q < NR; q++) my[q] = EP_NONE;                    // dependency.rs:113-137: no key, no dependencies
        }
        // max_seq_num (dependency.rs:101-109): the R sequence numbers in one round
        uint64_t ms = 0;
        bool ok[NR]; uint64_t sq[NR];
#pragma unroll
        for (int q = 0; q < NR; q++) {
            ok[q] = (uint32_t)q < v.R && my[q] != EP_NONE && L.held((uint32_t)q < v.R ? q : 0, my[q]);
            sq[q] = L.seq_at(L.ix((uint32_t)q < v.R ? q : 0, ok[q] ? my[q] : 0u));
        }
#pragma unroll
        for (int q = 0; q < NR; q++) if (ok[q] && sq[q] > ms) ms = sq[q];
        ms += 1;
        EPC_SUB(L, 3);
#pragma unroll
        for (int q = 0; q < NR; q++) {                                       // deps.union(&my_deps)
            if (in[q] != EP_NONE) { if (my[q] != EP_NONE && my[q] > in[q]) in[q] = my[q]; }
            else in[q] = my[q];
        }
        if (ms > s) s = ms;
    }
    L.note_rewrite(c, L.get_cb(row));
    I.bal = b; I.set_status(MODE == 2 ? EST_COMMITTED : (MODE == 1 ? EST_ACCEPTING : EST_PREACCEPTING));
    I.seq = s; I.set_key(k);
#pragma unroll
    for (int q = 0; q < NR; q++) I.d[q] = (uint32_t)q < v.R ? in[q] : EP_NONE;
    const uint32_t bk = I.bk();
    if (MODE != 2) I.set_bk((bk & 1u) | 2u | (src << 2));                    // replica_bk.source = peer
    EPC_SUB(L, 4);
    L.store_inst(i, I);
    if (rec) { *rec = I; *stored = true; }
    if (k != EP_NO_KEY && !hc_known && (hc_row == EP_NONE || c > hc_row)) EA(v.hc, SHL_OF(M24(g, v.n_keys) + k, v.hc_es) + row) = c;   // refresh_highest_cols, dependency.rs:141-167
    EPC_SUB(L, 5);
    if (MODE == 2) {
        L.logged_commit_slot(row, c, &I);                                    // durability.rs:104-135
    } else {
        if (LBK && (bk & 1u)) {                                              // durability.rs:25 / :78: leader_bk first
            if (MODE == 1) L.accept_reply(v.me, row, c, b); else L.pre_accept_reply(v.me, row, c, b, s, in, 0u);
        } else {
            of = 1; ob = b; os = s;
#pragma unroll
            for (int q = 0; q < NR; q++) d[q] = in[q];
        }
    }
}

template <int MODE, int NR, bool LBK, bool C>
__device__ __forceinline__ void ep_acceptor_lane(EpLaneT<NR, C> &L, bool on, uint32_t src, uint32_t row, uint32_t c, uint64_t b, uint64_t s,
                                                 const uint32_t *__restrict__ deps, uint32_t k, uint8_t &of, uint64_t &ob, uint64_t &os,
                                                 uint32_t (&d)[NR], EpInst<NR> *rec = nullptr, bool *stored = nullptr) {
    uint32_t in[NR];                                                         // round 1: the message's DepSet [R][G]
#pragma unroll
    for (int q = 0; q < NR; q++) in[q] = (uint32_t)q < L.v.R ? deps[(size_t)q * L.v.G + L.g] : EP_NONE;
    ep_acceptor_lane_in<MODE, NR, LBK, C>(L, on, src, row, c, b, s, in, k, of, ob, os, d, rec, stored);
}

template <int NR>
__global__ __launch_bounds__(256) void ep_execute_kernel(const EpView v, const EpExec x) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    EpLaneT<NR, false> L(v, g < v.G ? g : 0);
    EpExecLaneT<NR, false> E(v, x, L, L.g);
    if (g < v.G) ep_exec_after_handler(v, x, E);
    E.flush();
}

__global__ __launch_bounds__(256) void ep_propose_kernel(const EpView v, const uint8_t *__restrict__ key,
                                                         const uint8_t *__restrict__ exploded, uint8_t *__restrict__ m_flags,
                                                         uint32_t *__restrict__ m_col, uint64_t *__restrict__ m_seq,
                                                         uint32_t *__restrict__ m_deps) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    EpLane L(v, g < v.G ? g : 0);
    if (g < v.G) {
        uint8_t of; uint32_t oc; uint64_t os;
        uint32_t d[EMAXR];
        ep_propose_lane(L, key[g], exploded ? exploded[g] : 0u, of, oc, os, d);
        m_flags[g] = of; m_col[g] = oc; m_seq[g] = os;
#pragma unroll
        for (int i = 0; i < EMAXR; i++) if ((uint32_t)i < v.R) m_deps[(size_t)i * v.G + g] = d[i];
    }
    L.flush();
}

template <int MODE>
__global__ __launch_bounds__(256) void ep_acceptor_kernel(const EpView v, const uint8_t *__restrict__ flags,
                                                          const uint8_t *__restrict__ peer, const uint32_t *__restrict__ col,
                                                          const uint64_t *__restrict__ ballot, const uint64_t *__restrict__ seq,
                                                          const uint32_t *__restrict__ deps, const uint8_t *__restrict__ key,
                                                          uint8_t *__restrict__ r_flags, uint64_t *__restrict__ r_ballot,
                                                          uint64_t *__restrict__ r_seq, uint32_t *__restrict__ r_deps,
                                                          const uint8_t *__restrict__ rows) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    EpLane L(v, g < v.G ? g : 0);
    if (g < v.G) {
        uint8_t of = 0; uint64_t ob = 0, os = 0;
        uint32_t d[EMAXR];
#pragma unroll
        for (int i = 0; i < EMAXR; i++) d[i] = EP_NONE;
        if (flags[g] & 1) {
            const uint32_t src = peer[g];
            ep_acceptor_lane<MODE, EMAXR, true>(L, true, src, rows ? rows[g] : src, col[g], ballot[g], seq[g], deps, key[g], of, ob, os, d);   // (rows: an instance under explicit prepare)
        }
        if (MODE != 2) { r_flags[g] = of; r_ballot[g] = ob; }
        if (MODE == 0) {
            r_seq[g] = os;
#pragma unroll
            for (int i = 0; i < EMAXR; i++) if ((uint32_t)i < v.R) r_deps[(size_t)i * v.G + g] = d[i];
        }
    }
    L.flush();
}

// dependency.rs:175-240 fast_quorum_eligibility over a reply table held in registers (row p valid iff
// bit p of acks): 0 = undecided, else the Status to enter with (dseq, dd)
template <int NR>
__device__ __forceinline__ int ep_eval(const EpView &v, uint32_t acks, const uint64_t (&ps)[NR], const uint32_t (&pd)[NR][NR],
                                       uint32_t exploded, bool avoid, uint64_t &dseq, uint32_t (&dd)[NR]) {
    const uint32_t R = v.R, all_cnt = __popc(acks);
    if (all_cnt < v.simple_q) return 0;
    // dependency.rs:333-367 get_enough_identical: the largest class of equal (seq, deps)
    uint32_t max_cnt = 0; int best = -1;
#pragma unroll
    for (int p = 0; p < NR; p++) {
        if (!((acks >> p) & 1u)) continue;
        uint32_t same = 0;
#pragma unroll
        for (int q = 0; q < NR; q++) {
            bool eq = ((acks >> q) & 1u) && ps[q] == ps[p];
#pragma unroll
            for (int k = 0; k < NR; k++) eq = eq && pd[q][k] == pd[p][k];
            same += eq ? 1u : 0u;
        }
        if (same > max_cnt) { max_cnt = same; best = p; }
    }
    if (!avoid && max_cnt >= v.super_q) {                                    // fast path
        dseq = 0;
#pragma unroll
        for (int p = 0; p < NR; p++) if (p == best) dseq = ps[p];
#pragma unroll
        for (int k = 0; k < NR; k++) {
            dd[k] = EP_NONE;
#pragma unroll
            for (int p = 0; p < NR; p++) if (p == best) dd[k] = pd[p][k];
        }
        return EST_COMMITTED;
    }
    uint32_t bad = 0;
#pragma unroll
    for (int p = 0; p < NR; p++)
        if ((uint32_t)p < R && !((acks >> p) & 1u) && (uint32_t)p != v.me && ((exploded >> p) & 1u)) bad++;
    if (!avoid && max_cnt + (R - bad - all_cnt) >= v.super_q) return 0;      // :221-236 may still be reached
    dseq = 0;                                                                // slow path: max of seqs, union of deps
#pragma unroll
    for (int k = 0; k < NR; k++) dd[k] = EP_NONE;
#pragma unroll
    for (int p = 0; p < NR; p++) {
        if (!((acks >> p) & 1u)) continue;
        if (ps[p] > dseq) dseq = ps[p];
#pragma unroll
        for (int k = 0; k < NR; k++) {                                       // dependency.rs:85-97 union
            if (dd[k] != EP_NONE) { if (pd[p][k] != EP_NONE && pd[p][k] > dd[k]) dd[k] = pd[p][k]; }
            else dd[k] = pd[p][k];
        }
    }
    return EST_ACCEPTING;
}

// The PreAcceptReplies to the instance (row, c) I lead, applied in peer order (ctl) exactly as one
// handle_msg_pre_accept_reply call each (messages.rs:96-270) -- but on a register copy of the
// instance and of its reply table: the caller loads every incoming reply up front (in_f / in_b / in_s / in_d, row p = peer
// p's; my own row unused), the result is stored once.  dec = 0 / EST_ACCEPTING / EST_COMMITTED with (dseq, dd).
// (Loading every input row unconditionally from clamped addresses was measured SLOWER for this kernel -- 25.2 vs 21.7 us per
// launch, profiles/round2/r2w_ep_flat.log -- unlike the MultiPaxos tally's round 1; the variant is gone.)
// where the incoming replies lie: `RD::get(p, f, rb, rs, rd)` hands over peer p's (flag, ballot, seq, deps) -- out of register
// arrays the caller loaded (EpRepliesInRegs: the handler kernel), or out of the block's LDS (the one-launch tick)
template <int NR>
struct EpRepliesInRegs {
    const uint32_t (&in_f)[NR]; const uint64_t (&in_b)[NR]; const uint64_t (&in_s)[NR]; const uint32_t (&in_d)[NR][NR];
    __device__ __forceinline__ void get(uint32_t p, uint32_t &f, uint64_t &rb, uint64_t &rs, uint32_t (&rd)[NR]) const {
        f = 0; rb = 0; rs = 0;
#pragma unroll
        for (int k = 0; k < NR; k++) rd[k] = EP_NONE;
#pragma unroll
        for (int q = 0; q < NR; q++)
            if ((uint32_t)q == p) {
                f = in_f[q]; rb = in_b[q]; rs = in_s[q];
#pragma unroll
                for (int k = 0; k < NR; k++) rd[k] = in_d[q][k];
            }
    }
};

// own (ep_cluster_tick_pm_kernel): the instance as my proposal of this tick made it -- nothing of it or of my own reply is in memory
// yet (ep_propose_lane's rec_later): the record comes from *own_p, my reply is (own_p->seq, own_p->d), and whatever this call leaves
// behind goes out in full
template <int NR, bool C, typename RD>
__device__ __forceinline__ void ep_pa_replies_lane_rd(EpLaneT<NR, C> &L, uint32_t row, uint32_t c, uint32_t ctl, uint32_t ex, const RD &rdr,
                                                      uint8_t &dec, uint64_t &dseq, uint32_t (&dd)[NR],
                                                      EpInst<NR> *rec = nullptr, bool *stored = nullptr, const EpInst<NR> *own_p = nullptr,
                                                      bool own_on = true) {
    // (own_p names the caller's object whether or not this lane has an unmaterialized proposal -- own_on says that: a pointer
    // that is &object in some lanes and null in others kept the object in scratch, 44 B per lane)
    const bool own = own_p && own_on;
    const EpView &v = L.v;
    if (stored) *stored = false;
    const uint32_t R = v.R;
    const bool h = L.held(row, c);
    const uint32_t i = L.ix(row, c);
    // the instance (its ballot and meta words; the ring cell exists whether or not the column is still held) and the replies
    // it already holds
    EpInst<NR> I;
    I.make_null();
    if (own) I = *own_p;
    else { I.bal = L.bal_at(i); L.load_meta(i, I); }
    uint32_t st = h ? I.status() : 0u, acks = h ? I.pa_acks() : 0u;
    const uint64_t b = h ? I.bal : 0ull;
    const uint32_t bk = h ? I.bk() : 0u;
    const bool avoid = h && v.recovery && I.avoid();
    const uint32_t before = st, acks0 = acks;
    uint64_t ps[NR]; uint32_t pd[NR][NR];
#pragma unroll
    for (int p = 0; p < NR; p++) {
        const bool on = (acks >> p) & 1u, mine = own && (uint32_t)p == v.me;
        ps[p] = mine ? own_p->seq : (on ? EA(v.pa_seq, L.ps_ix(row, c, p)) : 0ull);
#pragma unroll
        for (int k = 0; k < NR; k++) pd[p][k] = mine ? own_p->d[k] : ((on && (uint32_t)k < R) ? EA(v.pa_deps, L.pd_ix(row, c, p, k)) : EP_NONE);
    }
    dseq = 0;
#pragma unroll
    for (int k = 0; k < NR; k++) dd[k] = EP_NONE;
    for (uint32_t oi = 0; oi < R; oi++) {
        const uint32_t p = (ctl >> (3 * oi)) & 7u;
        if (p == v.me || p >= R) continue;
        uint32_t f; uint64_t rb, rs; uint32_t rd[NR];
        rdr.get(p, f, rb, rs, rd);
        if (!(f & 1u) || !h) continue;
        if (st != EST_PREACCEPTING || (rb > 0 && b != rb) || !(bk & 1u)) continue;   // :129-134
        if ((acks >> p) & 1u) continue;                                      // :136-138
        if (rb > 0) {                                                        // :141-144
#pragma unroll
            for (int q = 0; q < NR; q++)
                if ((uint32_t)q == p) {
                    ps[q] = rs;
#pragma unroll
                    for (int k = 0; k < NR; k++) pd[q][k] = rd[k];
                }
            acks |= 1u << p;
        }
        const int next = ep_eval<NR>(v, acks, ps, pd, ex, avoid, dseq, dd);
        if (next) st = (uint32_t)next;
    }
    // write back: new replies, the ack mask, the decision.  (A reply is kept for the calls to come: once the instance has left
    // PreAccepting in THIS call nobody reads the table again -- a reader looks at acked peers of a PreAccepting instance only,
    // and fresh bookkeeping starts from an empty ack mask -- so the replies of a decided instance are not stored: 28 bytes per
    // peer, the common case of the one-launch tick, where all of an instance's replies arrive in one call.)
    const uint32_t fresh = own ? acks : (acks & ~acks0);                     // (own: my reply is not in the table either)
    const bool decided = h && before == EST_PREACCEPTING && st != EST_PREACCEPTING;
#pragma unroll
    for (int p = 0; p < NR; p++)
        if (((fresh >> p) & 1u) && !decided) {
            EA(v.pa_seq, L.ps_ix(row, c, p)) = ps[p];
#pragma unroll
            for (int k = 0; k < NR; k++)
                if ((uint32_t)k < R) EA(v.pa_deps, L.pd_ix(row, c, p, k)) = pd[p][k];
        }
    if (fresh) I.set_pa_acks(acks);
    dec = 0;
    if (h && before == EST_PREACCEPTING && st != EST_PREACCEPTING) {
        I.seq = dseq;
#pragma unroll
        for (int k = 0; k < NR; k++) I.d[k] = (uint32_t)k < R ? dd[k] : EP_NONE;
        I.set_status(st);
        L.store_inst(i, I);                                                  // (ballot unchanged, seq / deps / Status / ack mask new)
        if (rec && st == EST_COMMITTED) { *rec = I; *stored = true; }
        if (st == EST_COMMITTED) { L.n_fast++; L.logged_commit_slot(row, c, &I); dec = EST_COMMITTED; }   // :158-206
        else { L.n_slow++; L.accept_reply(v.me, row, c, b); dec = L.status_at(i) >= EST_COMMITTED ? EST_COMMITTED : EST_ACCEPTING; }   // :209-262
    } else if (own) {
        L.store_inst(i, I);                                                  // undecided: the proposal's record, with the acks so far, for the first time
    } else if (fresh) {
        L.store_meta(i, I);                                                  // only the ack mask moved (deps[4], deps[5] as loaded)
    }
}

template <int NR, bool C>
__device__ __forceinline__ void ep_pa_replies_lane(EpLaneT<NR, C> &L, uint32_t row, uint32_t c, uint32_t ctl, uint32_t ex,
                                                   const uint32_t (&in_f)[NR], const uint64_t (&in_b)[NR], const uint64_t (&in_s)[NR],
                                                   const uint32_t (&in_d)[NR][NR], uint8_t &dec, uint64_t &dseq, uint32_t (&dd)[NR],
                                                   EpInst<NR> *rec = nullptr, bool *stored = nullptr) {
    const EpRepliesInRegs<NR> rdr{in_f, in_b, in_s, in_d};
    ep_pa_replies_lane_rd<NR, C>(L, row, c, ctl, ex, rdr, dec, dseq, dd, rec, stored);
}

template <int NR>
__global__ __launch_bounds__(256) void ep_pre_accept_replies_kernel(const EpView v, const uint32_t *__restrict__ col,
                                                                    const uint64_t *__restrict__ ballot,
                                                                    const uint64_t *__restrict__ seq,
                                                                    const uint32_t *__restrict__ deps,
                                                                    const uint8_t *__restrict__ flags,
                                                                    const uint32_t *__restrict__ order,
                                                                    const uint8_t *__restrict__ exploded,
                                                                    uint8_t *__restrict__ decision, uint64_t *__restrict__ d_seq,
                                                                    uint32_t *__restrict__ d_deps, const uint8_t *__restrict__ rows) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    EpLaneT<NR> L(v, g < v.G ? g : 0);
    if (g < v.G) {
        const uint32_t R = v.R;
        uint32_t in_f[NR]; uint64_t in_b[NR], in_s[NR]; uint32_t in_d[NR][NR];
#pragma unroll
        for (int p = 0; p < NR; p++) {
            const bool on = (uint32_t)p < R && (uint32_t)p != v.me;
            const size_t o = (size_t)p * v.G + g;
            in_f[p] = on ? flags[o] : 0u; in_b[p] = on ? ballot[o] : 0ull; in_s[p] = on ? seq[o] : 0ull;
#pragma unroll
            for (int k = 0; k < NR; k++) in_d[p][k] = (on && (uint32_t)k < R) ? deps[((size_t)p * R + k) * v.G + g] : EP_NONE;
        }
        uint8_t dec; uint64_t dseq; uint32_t dd[NR];
        ep_pa_replies_lane(L, (rows && rows[g] < R) ? rows[g] : v.me, col[g], order ? order[g] : SMR_CTL_IDENTITY,
                               exploded ? exploded[g] : 0u, in_f, in_b, in_s, in_d, dec, dseq, dd);
        decision[g] = dec; d_seq[g] = dec ? dseq : 0ull;
#pragma unroll
        for (int k = 0; k < NR; k++) if ((uint32_t)k < R) d_deps[(size_t)k * v.G + g] = dec ? dd[k] : EP_NONE;
    }
    L.flush();
}

// ---- the command leader's receive side of a tick in ONE launch ---------------------------------------------------------------------
// smr_wire_ingest_ep_pre_accept_replies parses the acceptors' connections into ballot / seq / flags [R][G] and deps [R][R][G]
// (two memsets in front: the flag plane, the counters) and smr_ep_handle_pre_accept_replies reads them back: four stream operations
// and, at R = 5, 37 bytes per connection out and in again for frames of 25 to 45 bytes.  Here the parse is the prologue of the
// handler, as raft_wire_replies_kernel's is of the Raft leader's.  The connections come DENSE: connection c = g * (R - 1) + k is
// group g's k-th peer (ids ascending, my own left out), so a block's EW_BLOCK / (R - 1) groups have all their connections in the
// block.  Every lane walks its connection out of the block's LDS copy of the buffer span (wire_rd.h; the rules are the WR_EPAXOS arm
// of wire_ingest_replies_kernel: same reply taken, same frames located, same `consumed` / `status`) and leaves the reply it takes
// in LDS, [peer slot][group of the block]: ballot, seq, R dependencies, a flag.  A reply that did not come is a flag of zero; no
// array in between, nothing to zero.  Behind one barrier the block's first lanes run ep_pa_replies_lane_rd on their group
// (messages.rs:96-270) with an RD that reads those words.
// Own row only: the instances a replica leads outside its row under explicit prepare (row_dev, the _at entries) stay with the two calls.
//
// 512 lanes per block: stage 20 KB + located frames 6 KB + reply words 37 B (NR = 5) / 49 B (NR = 8) per lane = 45.5 / 51.6 KB of
// LDS, three blocks per CU (raft_wire_replies_kernel's 1024 lanes and 77 KB leave one).
//
// The call's four counters: summed per block in LDS, added into a scratch of the replica's (16 shards of the three plain
// counters; the located frames' places come from one word), handed out by the block whose arrival is the grid's last (arrival
// tickets in two levels of <= 32 arrivals each, as raft_wire_replies_kernel's: a same-address atomic is ~10-25 ns and there
// are 512 blocks).  NOTHING in that scratch is ever reset, so no call can leave it dirty for the next one: every word only
// counts up.  A ticket word receives the same number of arrivals in every call of a replica (the grid is the replica's), so
// "last" is "the count after mine is a multiple of that number"; the counters are cumulative and the last block hands out the
// difference to the totals the previous call's last block left in snap[] (written with atomicMax: cumulative totals only grow).
// A launch that never ran added nothing; two calls that overlapped against the contract (one stream at a time per replica)
// get each other's counts, and the call after them is exact again.  The entry point zeroes the scratch on its error returns.
// "My adds before my ticket, the last block reads everyone's adds" is ordered by fences: an agent-scope release (__threadfence)
// in front of every ticket, an acquire behind every winning one.
struct EpWire {
    const uint8_t *buf; uint64_t buf_len;
    const uint64_t *conn_off; const uint8_t *conn_len; uint32_t n_conn;
    const uint32_t *col, *order; const uint8_t *exploded;
    uint8_t *decision; uint64_t *d_seq; uint32_t *d_deps;
    smr_wire_other *others; uint64_t other_cap;
    uint64_t *counts, *consumed; int32_t *status;
    unsigned long long *acc;                     // the replica's, cumulative: [0] top ticket, [1] located frames, [2 .. 5] snap[4]: the four counters'
};                                               //  totals as the last call left them, [8 ..) the shards, then 64 level-1 tickets
#ifndef EW_BLOCK_N
#define EW_BLOCK_N 512           // (lanes per block; 1024 would need 91 KB of LDS at NR = 5: one block per CU, what bounds the Raft kernel)
#endif
constexpr uint32_t EW_BLOCK = EW_BLOCK_N, EW_STAGE = EW_BLOCK * 40, EW_LOC = EW_BLOCK / 2;
constexpr uint32_t EW_SHARDS = 16, EW_TICK1 = 8 + EW_SHARDS * 4, EW_ACC_WORDS = EW_TICK1 + 64;
__device__ __forceinline__ unsigned long long ew_read(unsigned long long *w) { return atomicAdd(w, 0ull); }   // (at L2, where the atomics are)

// the replies a block parsed, in its LDS: peer p's reply to group `gi` of the block lies at [slot of p][gi]
template <int NR>
struct EpRepliesInWireLds {
    const uint64_t *bal, *seq; const uint32_t (*dep)[EW_BLOCK]; const uint8_t *fl;
    uint32_t me, R, gpb, gi;
    __device__ __forceinline__ void get(uint32_t p, uint32_t &f, uint64_t &rb, uint64_t &rs, uint32_t (&rd)[NR]) const {
        const uint32_t i = (p - (p > me ? 1u : 0u)) * gpb + gi;             // (p != me: the caller skips the leader itself)
        f = fl[i];
        rb = f ? bal[i] : 0ull; rs = f ? seq[i] : 0ull;
#pragma unroll
        for (int k = 0; k < NR; k++) rd[k] = (f && (uint32_t)k < R) ? dep[k][i] : EP_NONE;
    }
};

template <int NR>
__global__ __launch_bounds__(EW_BLOCK) void ep_wire_pre_accept_replies_kernel(const EpView v, const EpWire A) {
    __shared__ uint32_t stage[EW_STAGE / 4 + 4];
    __shared__ smr_wire_other loc[EW_LOC];
    __shared__ uint32_t blk[4];
    __shared__ unsigned long long loc_base;
    __shared__ uint64_t sh_bal[EW_BLOCK], sh_seq[EW_BLOCK];
    __shared__ uint32_t sh_dep[NR][EW_BLOCK];
    __shared__ uint8_t sh_fl[EW_BLOCK];
    if (threadIdx.x < 4) blk[threadIdx.x] = 0;
    const unsigned long long loc_before = A.acc[3];                           // snap[1]: the located frames of all calls before this one
    const uint32_t F = v.R - 1u, GPB = EW_BLOCK / F;                          // peers per group, groups per block
    const uint32_t g0 = blockIdx.x * GPB, c0 = g0 * F;
    const uint32_t n_here = (A.n_conn - c0) < GPB * F ? (A.n_conn - c0) : GPB * F;
    const bool live = threadIdx.x < n_here;
    const uint32_t c = c0 + threadIdx.x;
    const uint64_t start = live ? A.conn_off[c] : 0, end = !live ? 0 : A.conn_len ? start + A.conn_len[c] : A.conn_off[c + 1];
    // my block's span of the buffer -> LDS: from its first connection's start (16-byte aligned down) as far as the stage goes
    const uint32_t c1 = c0 + n_here;
    const uint64_t s0 = A.conn_off[c0] & ~15ull, s1 = A.conn_len ? A.conn_off[c1 - 1] + A.conn_len[c1 - 1] : A.conn_off[c1];
    uint64_t slo = 0, shi = 0;
    if (s0 < s1 && s1 <= A.buf_len) {
        slo = s0; shi = s1 - s0 <= EW_STAGE ? s1 : s0 + EW_STAGE;
        const uint32_t n16 = (uint32_t)((shi - slo + 15) / 16);
        for (uint32_t i = threadIdx.x; i <= n16; i += EW_BLOCK) {                  // (one chunk more: the dwords a read at the last bytes reaches into)
            const uint64_t off = slo + 16ull * i;
            uint32_t w[4] = {0, 0, 0, 0};
            if (off + 16 <= A.buf_len) {
                const wr_u32x4 x = *(const wr_u32x4 *)(A.buf + off);
                w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
            } else {
                for (uint32_t b = 0; b < 16 && off + b < A.buf_len; b++) w[b >> 2] |= (uint32_t)A.buf[off + b] << (8 * (b & 3));
            }
            if (4 * i + 3 < EW_STAGE / 4 + 4) { stage[4 * i] = w[0]; stage[4 * i + 1] = w[1]; stage[4 * i + 2] = w[2]; stage[4 * i + 3] = w[3]; }
        }
    }
    sh_fl[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t my_gi = threadIdx.x / F, my_k = threadIdx.x - my_gi * F;
    const uint32_t my_w = my_k * GPB + my_gi;                                   // where my connection's reply goes: [peer slot][group of the block]
    const uint32_t my_col = live ? A.col[g0 + my_gi] : 0u;
    uint64_t pos = start;
    int st = 0;
    bool have = false, deferred = false;
    if (live && (end < start || end > A.buf_len)) st = 1;
    while (live && st == 0) {
        const uint64_t avail = end - pos;
        if (avail < 8) break;                                                       // length not complete yet
        GlRd r{A.buf, pos, pos + 8, A.buf_len, true, stage, slo, shi};
        const uint64_t plen = __builtin_bswap64(r.peek64());
        if (plen > 1000000000000ull) { st = 1; break; }                             // safetcp.rs:56-66
        if (avail - 8 < plen) break;                                                // frame not complete yet
        r.n = pos + 8; r.end = pos + 8 + plen;
        uint32_t kind = SMR_WIRE_OTHER;
        bool mine = false;
        const uint64_t outer = r.varint();
        if (outer == 2) kind = SMR_WIRE_LEAVE;                                      // PeerMessage::Leave
        else if (outer == 0) {                                                      // PeerMessage::Msg { msg }
            const uint64_t var = r.varint();
            if (!r.ok) { st = 1; break; }
            kind = (uint32_t)(var <= SMR_WIRE_EP_COMMIT_NOTICE ? var : SMR_WIRE_OTHER);   // (ExpPrepare & co, Heartbeat: located)
            if (var == SMR_WIRE_EP_PRE_ACCEPT_REPLY) {
                uint8_t row; uint64_t col, ballot, seq, n; bool fits;
                // (the dependencies go straight to my LDS words while no reply is taken yet -- they count only under the flag,
                //  and a reply that turns out not to be mine leaves the flag as it is; behind a taken reply they go nowhere)
                const bool keep = !have;
                if (!wr_ep_pre_accept_reply(r, row, col, ballot, seq, n, fits, [&](uint32_t q, uint32_t x) {
                        if (keep && q < (uint32_t)NR && q < v.R) sh_dep[q][my_w] = x;
                    })) { st = 1; break; }
                mine = row == v.me && col == (uint64_t)my_col && n == v.R && fits;
                if (mine) {
                    if (have) { deferred = true; break; }                           // the next call's
                    sh_bal[my_w] = ballot; sh_seq[my_w] = seq; sh_fl[my_w] = 1;
                    have = true;
                }
            }
        }
        if (!r.ok) { st = 1; break; }                                               // (the enum tags did not parse)
        if (!mine) {                                                                // located, not validated
            smr_wire_other o; o.conn = c; o.kind = kind; o.off = pos; o.len = 8 + plen;
            const uint32_t at = atomicAdd(&blk[1], 1u);
            if (at < EW_LOC) loc[at] = o;
            else {                                                                  // (more than the block keeps: straight to the call's list)
                const unsigned long long far = atomicAdd(&A.acc[1], 1ull) - loc_before;
                if (far < A.other_cap) A.others[far] = o;
            }
        }
        pos += 8 + plen;
    }
    if (live) {
        A.consumed[c] = st ? 0 : pos - start;                                       // (a malformed connection: the host looks at all of it)
        A.status[c] = st;                                                           // (a reply taken in front of the malformed frame stays
    }                                                                               //  taken, as its flag stays set after the two calls)
    const unsigned long long m0 = __ballot(have && st == 0), m2 = __ballot(st != 0), m3 = __ballot(deferred);
    if (threadIdx.x % 64 == 0) {
        if (m0) atomicAdd(&blk[0], (uint32_t)__popcll(m0));
        if (m2) atomicAdd(&blk[2], (uint32_t)__popcll(m2));
        if (m3) atomicAdd(&blk[3], (uint32_t)__popcll(m3));
    }
    __syncthreads();
    // (the located frames' place in the call's list: asked for NOW, used behind the handler -- the word is one for all blocks)
    const uint32_t n_kept = blk[1] < EW_LOC ? blk[1] : EW_LOC;
    unsigned long long my_base = 0;
    if (threadIdx.x == 0 && n_kept) my_base = atomicAdd(&A.acc[1], (unsigned long long)n_kept) - loc_before;
    // ---- the handler: one lane per group of the block, its peers' replies out of LDS ----
    const uint32_t g = g0 + threadIdx.x;
    const bool leads = threadIdx.x < GPB && g < v.G;
    EpLaneT<NR> L(v, leads ? g : 0);
    if (leads) {
        const EpRepliesInWireLds<NR> rdr{sh_bal, sh_seq, sh_dep, sh_fl, v.me, v.R, GPB, threadIdx.x};
        uint8_t dec; uint64_t dseq; uint32_t dd[NR];
        ep_pa_replies_lane_rd<NR, false>(L, v.me, A.col[g], A.order ? A.order[g] : SMR_CTL_IDENTITY, A.exploded ? A.exploded[g] : 0u, rdr, dec, dseq, dd);
        A.decision[g] = dec; A.d_seq[g] = dec ? dseq : 0ull;
#pragma unroll
        for (int k = 0; k < NR; k++) if ((uint32_t)k < v.R) A.d_deps[(size_t)k * v.G + g] = dec ? dd[k] : EP_NONE;
    }
    if ((threadIdx.x & ~63u) < GPB) L.flush();                                      // (the wavefronts that hold a handler lane)
    // ---- the call's counters: this block's share, the located frames' place, and -- the last block -- the totals ----
    if (threadIdx.x == 0) {
        unsigned long long *const shard = A.acc + 8 + (blockIdx.x % EW_SHARDS) * 4u;
        if (blk[0]) atomicAdd(&shard[0], (unsigned long long)blk[0]);
        if (blk[2]) atomicAdd(&shard[2], (unsigned long long)blk[2]);
        if (blk[3]) atomicAdd(&shard[3], (unsigned long long)blk[3]);
        loc_base = my_base;
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < n_kept; j += EW_BLOCK)
        if (loc_base + j < A.other_cap) A.others[loc_base + j] = loc[j];
    if (threadIdx.x == 0) {
        // arrivals: my level-1 ticket (blocks 32 k .. 32 k + 31), its last arrival goes on to the top ticket; the last of all hands the totals out
        const uint32_t n1 = (gridDim.x + 31u) / 32u, t1 = blockIdx.x / 32u;
        const uint32_t mine = t1 + 1u < n1 ? 32u : gridDim.x - 32u * (n1 - 1u);
        bool last = false;
        __threadfence();                                                            // release: my block's adds are in front of my ticket
        if (n1 > 64u) last = (atomicAdd(&A.acc[0], 1ull) + 1ull) % gridDim.x == 0ull;   // (more level-1 groups than tickets: one level)
        else if ((atomicAdd(&A.acc[EW_TICK1 + t1], 1ull) + 1ull) % mine == 0ull) {
            __threadfence();                                                        // acquire my group's, release towards the top ticket
            last = (atomicAdd(&A.acc[0], 1ull) + 1ull) % n1 == 0ull;
        }
        if (last) {
            __threadfence();                                                        // acquire: every other block's adds are behind its ticket
            unsigned long long tot[4] = {0ull, 0ull, 0ull, 0ull};
            for (uint32_t sh = 0; sh < EW_SHARDS; sh++)
#pragma unroll
                for (int q = 0; q < 4; q++) if (q != 1) tot[q] += ew_read(&A.acc[8 + sh * 4 + q]);
            tot[1] = ew_read(&A.acc[1]);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                A.counts[q] = tot[q] - ew_read(&A.acc[2 + q]);
                atomicMax(&A.acc[2 + q], tot[q]);
            }
        }
    }
}

// the AcceptReplies to the instance (row, c) I lead: flags / ballot rows by peer (stride G), peers in ctl order, one
// handle_msg_accept_reply each (messages.rs:348-436); true = the instance went from Accepting to Committed here
template <int NR, bool C>
__device__ __forceinline__ bool ep_accept_replies_lane(EpLaneT<NR, C> &L, uint32_t row, uint32_t c, uint32_t ctl,
                                                       const uint8_t *__restrict__ flags, const uint64_t *__restrict__ ballot,
                                                       uint64_t fixed_ballot) {
    const EpView &v = L.v;
    const uint32_t R = v.R;
    const bool h = L.held(row, c);
    const uint32_t before = h ? L.status_at(L.ix(row, c)) : 0u;
    for (uint32_t oi = 0; oi < R; oi++) {
        const uint32_t p = (ctl >> (3 * oi)) & 7u;
        if (p == v.me || p >= R) continue;
        const size_t o = (size_t)p * v.G + L.g;
        if (!(flags[o] & 1)) continue;
        L.accept_reply(p, row, c, ballot ? ballot[o] : fixed_ballot);
    }
    return h && before == EST_ACCEPTING && L.status_at(L.ix(row, c)) >= EST_COMMITTED;
}

// the same with the replies as a bit mask (bit p: peer p answered, with the Accept's ballot `fixed_ballot`): the one-launch tick
template <int NR, bool C>
__device__ __forceinline__ bool ep_accept_replies_mask(EpLaneT<NR, C> &L, uint32_t row, uint32_t c, uint32_t ctl, uint32_t fmask, uint64_t fixed_ballot) {
    const EpView &v = L.v;
    const uint32_t R = v.R;
    const bool h = L.held(row, c);
    const uint32_t before = h ? L.status_at(L.ix(row, c)) : 0u;
    for (uint32_t oi = 0; oi < R; oi++) {
        const uint32_t p = (ctl >> (3 * oi)) & 7u;
        if (p == v.me || p >= R || !((fmask >> p) & 1u)) continue;
        L.accept_reply(p, row, c, fixed_ballot);
    }
    return h && before == EST_ACCEPTING && L.status_at(L.ix(row, c)) >= EST_COMMITTED;
}

__global__ __launch_bounds__(256) void ep_accept_replies_kernel(const EpView v, const uint32_t *__restrict__ col,
                                                                const uint64_t *__restrict__ ballot,
                                                                const uint8_t *__restrict__ flags,
                                                                const uint32_t *__restrict__ order,
                                                                uint8_t *__restrict__ committed, const uint8_t *__restrict__ rows) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    EpLane L(v, g < v.G ? g : 0);
    if (g < v.G)
        committed[g] = ep_accept_replies_lane(L, (rows && rows[g] < v.R) ? rows[g] : v.me, col[g], order ? order[g] : SMR_CTL_IDENTITY,
                                              flags, ballot, 0ull) ? 1 : 0;
    L.flush();
}

// ---- explicit prepare --------------------------------------------------------------------------------------------------
// heartbeat.rs:17-125 for HearTimeout { peer = src[g] } (SMR_NO_REPLICA: none in this group)
// EXEC (smr_ep_cfg.execute with recovery): this one call runs SEVERAL inner handlers per group -- a PreAcceptReply per waiting
// instance, then my own ExpPrepareReplies -- and each may move a commit bar, so the attempts and results the reference runs
// behind each of them (durability.rs:136-160, LS-1 rule 0) run here, right behind each, in the reference's order; the
// separate ep_execute_kernel (one moved bar per call) stays what every other handler uses
template <bool EXEC>
__global__ __launch_bounds__(256) void ep_heartbeat_timeout_kernel(const EpView v, const EpExec x, const uint8_t *__restrict__ src,
                                                                   const uint8_t *__restrict__ exploded, uint32_t *__restrict__ out_n,
                                                                   uint32_t *__restrict__ out_col, uint64_t *__restrict__ out_bal) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    EpLane L(v, g < v.G ? g : 0);
    EpExecLane E(v, x, L, L.g);
    if (g < v.G) {
        const uint32_t ts = src[g], R = v.R;
        uint32_t n = 0;
        if (ts < R && ts != v.me) {
            const uint32_t ex = exploded ? exploded[g] : 0u;
            uint32_t none[EMAXR];
#pragma unroll
            for (int k = 0; k < EMAXR; k++) none[k] = EP_NONE;
            // :35-60 every PreAccepting instance I lead, from its row's commit bar: "reply" with ballot 0
            for (uint32_t row = 0; row < R; row++) {
                const uint32_t end = L.get_len(row);
                for (uint32_t c = L.get_cb(row); c < end; c++) {
                    if (!L.held(row, c)) continue;
                    const uint32_t i = L.ix(row, c);
                    EpInst<EMAXR> J;
                    L.load_meta(i, J);
                    if (J.status() == EST_PREACCEPTING && (J.bk() & 1)) {
                        L.pre_accept_reply(ts, row, c, 0, 0, none, ex);
                        if (EXEC) E.after_inner_handler();
                    }
                }
            }
            // :62-107 ExpPrepare for every in-progress instance of that peer's row (exec bars: 0 without execution)
            const uint32_t row = ts, end = L.get_len(row);
            for (uint32_t c = end > v.W ? end - v.W : 0u; c < end; c++) {
                const uint32_t i = L.ix(row, c);
                EpInst<EMAXR> J;
                L.load_meta(i, J);
                const uint32_t st = J.status(), bk = J.bk();
                if (st >= EST_EXECUTING || ((bk & 2u) && ((bk >> 2) & 7u) != ts)) continue;   // :73-80
                if (st == EST_COMMITTED) continue;                               // :82-84
                const uint64_t nb = (((L.bal_at(i) >> 8) + 1) << 8) | (uint64_t)(v.me + 1);   // make_greater_ballot, mod.rs:500-508
                L.fresh_leader_bk(i, J);
                L.store_meta(i, J);
                out_col[(size_t)n * v.G + g] = c; out_bal[(size_t)n * v.G + g] = nb;
                n++;
            }
            // :110-123 my own ExpPrepareReplies
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t c = out_col[(size_t)k * v.G + g];
                const uint32_t i = L.ix(row, c);
                const EpInst<EMAXR> J = L.load_inst(i);
                uint32_t d[EMAXR];
#pragma unroll
                for (int q = 0; q < EMAXR; q++) d[q] = (uint32_t)q < R ? J.d[q] : EP_NONE;
                L.exp_prepare_reply(v.me, row, c, out_bal[(size_t)k * v.G + g], J.bal, J.status(), J.seq, d, J.key());
                if (EXEC) E.after_inner_handler();
            }
        }
        out_n[g] = n;
        if (EXEC) EA(x.n_sub, g) = E.n_order;
    }
    L.flush();
    if (EXEC) E.flush();
}

// messages.rs:511-574: one ExpPrepare { slot = (row, col), new_ballot } from `peer` per group; the ExpPrepareReply back
__global__ __launch_bounds__(256) void ep_exp_prepare_kernel(const EpView v, const uint8_t *__restrict__ flags,
                                                             const uint8_t *__restrict__ peer, const uint8_t *__restrict__ rows,
                                                             const uint32_t *__restrict__ col, const uint64_t *__restrict__ nbal,
                                                             uint8_t *__restrict__ r_flags, uint64_t *__restrict__ r_vbal,
                                                             uint8_t *__restrict__ r_status, uint64_t *__restrict__ r_seq,
                                                             uint32_t *__restrict__ r_deps, uint8_t *__restrict__ r_key) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= v.G) return;
    EpLane L(v, g);
    uint8_t of = 0, ost = 0, ok = EP_NO_KEY; uint64_t ob = 0, os = 0;
    uint32_t d[EMAXR];
#pragma unroll
    for (int q = 0; q < EMAXR; q++) d[q] = EP_NONE;
    if (flags[g] & 1) {
        const uint32_t row = rows[g], c = col[g];
        if (row < v.R && !(c < L.get_len(row) && !L.held(row, c))) {
            while (L.get_len(row) <= c) L.push_null(row);                        // :530-533
            const uint32_t i = L.ix(row, c);
            EpInst<EMAXR> J = L.load_inst(i);
            if (nbal[g] > J.bal) {                                               // :537
                J.set_bk((J.bk() & 1u) | 2u | ((uint32_t)peer[g] << 2));         // replica_bk.source = peer
                L.store_meta(i, J);
                of = 1; ob = J.bal; ost = (uint8_t)J.status(); os = J.seq; ok = (uint8_t)J.key();
#pragma unroll
                for (int q = 0; q < EMAXR; q++) d[q] = (uint32_t)q < v.R ? J.d[q] : EP_NONE;
            }
        }
    }
    r_flags[g] = of; r_vbal[g] = ob; r_status[g] = ost; r_seq[g] = os; r_key[g] = ok;
#pragma unroll
    for (int q = 0; q < EMAXR; q++) if ((uint32_t)q < v.R) r_deps[(size_t)M24(q, v.G) + g] = d[q];
}

// The ExpPrepareReplies to the instance (rows[g], col[g]) I am preparing, one handle_msg_exp_prepare_reply each, peers in
// order[g] order; decision[g] = the Status of the message broadcast here (0: none) with its ballot / seq / deps / key
__global__ __launch_bounds__(256) void ep_exp_prepare_replies_kernel(const EpView v, const uint8_t *__restrict__ rows,
                                                                     const uint32_t *__restrict__ col, const uint64_t *__restrict__ nbal,
                                                                     const uint64_t *__restrict__ vbal, const uint8_t *__restrict__ vstatus,
                                                                     const uint64_t *__restrict__ vseq, const uint32_t *__restrict__ vdeps,
                                                                     const uint8_t *__restrict__ vkey, const uint8_t *__restrict__ flags,
                                                                     const uint32_t *__restrict__ order, uint8_t *__restrict__ decision,
                                                                     uint64_t *__restrict__ d_bal, uint64_t *__restrict__ d_seq,
                                                                     uint32_t *__restrict__ d_deps, uint8_t *__restrict__ d_key) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    EpLane L(v, g < v.G ? g : 0);
    if (g < v.G) {
        const uint32_t row = rows[g], c = col[g], R = v.R;
        const uint32_t ctl = order ? order[g] : SMR_CTL_IDENTITY;
        uint8_t dec = 0, dk = EP_NO_KEY; uint64_t db = 0, ds = 0;
        uint32_t dd[EMAXR];
#pragma unroll
        for (int q = 0; q < EMAXR; q++) dd[q] = EP_NONE;
        for (uint32_t oi = 0; oi < R && row < R; oi++) {
            const uint32_t p = (ctl >> (3 * oi)) & 7u;
            if (p == v.me || p >= R) continue;
            const size_t o = (size_t)p * v.G + g;
            if (!(flags[o] & 1)) continue;
            uint32_t d[EMAXR];
#pragma unroll
            for (int q = 0; q < EMAXR; q++) d[q] = (uint32_t)q < R ? vdeps[((size_t)p * R + q) * v.G + g] : EP_NONE;
            const int next = L.exp_prepare_reply(p, row, c, nbal[o], vbal[o], vstatus[o], vseq[o], d, vkey[o]);
            if (next) {
                const EpInst<EMAXR> J = L.load_inst(L.ix(row, c));
                dec = (uint8_t)next; db = nbal[o]; ds = J.seq; dk = (uint8_t)J.key();
#pragma unroll
                for (int q = 0; q < EMAXR; q++) dd[q] = (uint32_t)q < R ? J.d[q] : EP_NONE;
            }
        }
        decision[g] = dec; d_bal[g] = db; d_seq[g] = ds; d_key[g] = dk;
#pragma unroll
        for (int q = 0; q < EMAXR; q++) if ((uint32_t)q < R) d_deps[(size_t)M24(q, v.G) + g] = dd[q];
    }
    L.flush();
}

}  // namespace smr

using namespace smr;

struct smr_ep_replica {
    smr_ep_cfg cfg;
    EpView v;
    EpExec x;
    Arena arena;
    bool skip_exec = false;      // smr_ep_cluster_tick around the handlers that cannot move a commit bar (see there)
    smr_ep_replica **seat = nullptr;   // my seat in the cluster whose per-key table I use (smr_ep_cluster_create): cleared when I go first
    unsigned long long *wire_acc = nullptr;   // smr_ep_leader_handle_wire_pre_accept_replies: its counters and arrival tickets, cumulative over the calls
    SnapGroupListBuf glist;      // smr_ep_reset_groups' list on the device
};

namespace smr {
template <typename T> static void ecarve(Arena &a, T *&p, size_t n, bool dry) {
    size_t off = a.reserve(n * sizeof(T));
    if (!dry) p = a.at<T>(off);
}
static void ep_layout(smr_ep_replica *e, bool dry) {
    Arena &a = e->arena;
    a.used = 0;
    EpView &v = e->v;
    const size_t G = e->cfg.n_groups, W = e->cfg.window, R = e->cfg.population, K = e->cfg.n_keys;
    ecarve(a, v.p0, R * W * G, dry); ecarve(a, v.p1, R * W * G, dry); ecarve(a, v.p2, R * W * G, dry);
    if (R > 6) ecarve(a, v.p3, R * W * G, dry);
    ecarve(a, v.sq32, R * W * G, dry);
    const size_t PR = e->cfg.recovery ? R : 1;                                   // reply tables: every row / my row only
    ecarve(a, v.pa_seq, PR * W * R * G, dry); ecarve(a, v.pa_deps, PR * W * R * R * G, dry);
    if (e->cfg.recovery) {
        ecarve(a, v.xp_max, R * W * G, dry);
        ecarve(a, v.xv_status, R * W * R * G, dry); ecarve(a, v.xv_key, R * W * R * G, dry); ecarve(a, v.xv_seq, R * W * R * G, dry);
        ecarve(a, v.xv_deps, R * W * R * R * G, dry);
    }
    ecarve(a, v.len, R * G, dry); ecarve(a, v.commit_bars, R * G, dry); ecarve(a, v.my_nulls, G, dry); ecarve(a, v.rewritten, G, dry);
    ecarve(a, v.hc, K * (size_t)(R <= 6 ? 8 : 16) * G, dry);
    ecarve(a, v.counters, SMR_CTR_WORDS, dry);
    if (e->cfg.execute) {
        EpExec &x = e->x;
        ecarve(a, x.exec_bars, R * G, dry); ecarve(a, x.prev_cb, R * G, dry);
        ecarve(a, x.digest, G, dry);
        ecarve(a, x.node_of, R * W * G, dry); ecarve(a, x.nslot, R * W * G, dry); ecarve(a, x.head, R * W * G, dry);
        ecarve(a, x.sib, R * W * G, dry); ecarve(a, x.parent, R * W * G, dry);
        ecarve(a, x.order, 2 * R * W * G, dry); ecarve(a, x.n_sub, G, dry);
        ecarve(a, x.counters, SMR_CTR_WORDS, dry);
    }
}
// ---- the closed loop of a co-located cluster (smr_ep_cluster_*): the little flag arithmetic between the handlers ----------
// A cluster's replicas share ONE per-key table (round 5): entry (g, key) is a 128-byte line, replica q's R + 1 words (the key's
// highest column in each row, the executor's KV word) at word q * (R + 1) of it.  The five replica-wavefronts of a tick's block
// look a key up in the same steps: one line in, one line out per (group, key) where five private tables moved five
// (profiles/r5v: the entries' lines were most of the tick's 10x traffic).  to_shared: private entries -> slots; else back.
__global__ __launch_bounds__(256) void ep_hc_migrate_kernel(uint32_t *__restrict__ priv, uint32_t priv_es, uint32_t priv_kv, uint32_t *__restrict__ slot0,
                                                            uint32_t shared_es, uint32_t R, uint32_t n_entries, int to_shared) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_entries) return;
    uint32_t *a = priv + (size_t)e * priv_es, *b = slot0 + (size_t)e * shared_es;
    for (uint32_t w = 0; w <= R; w++) {
        const uint32_t pw = w < R ? w : priv_kv;                            // (the slot keeps its KV word right behind the R columns)
        if (to_shared) b[w] = a[pw]; else a[pw] = b[w];
    }
}

__global__ __launch_bounds__(256) void ep_init_records_kernel(u32x4 *__restrict__ p1, u32x4 *__restrict__ p2, u32x4 *__restrict__ p3, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    p1[i] = ep_init_p1();                                        // (ep_snapshot.h: what a new replica object holds; p0 is zero bytes)
    p2[i] = ep_init_p2();
    if (p3) p3[i] = ep_init_p3();
}
// out[g] = in[g] unless drop[g] (a lost message)
__global__ __launch_bounds__(256) void ep_flags_drop_kernel(uint32_t G, const uint8_t *__restrict__ in, const uint8_t *__restrict__ drop,
                                                            uint8_t *__restrict__ out) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g < G) out[g] = drop[g] ? 0 : in[g];
}
// out[g] = (a[g] == va) | (b != NULL && b[g] == vb)
__global__ __launch_bounds__(256) void ep_flags_eq_kernel(uint32_t G, const uint8_t *__restrict__ a, uint8_t va, const uint8_t *__restrict__ b,
                                                          uint8_t vb, uint8_t *__restrict__ out) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g < G) out[g] = (uint8_t)((a[g] == va) || (b && b[g] == vb));
}
__global__ __launch_bounds__(256) void ep_fill_kernel(uint32_t G, uint8_t *__restrict__ p8, uint8_t v8, uint64_t *__restrict__ p64, uint64_t v64) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g < G) { p8[g] = v8; p64[g] = v64; }
}

// ---- one tick of a co-located cluster in ONE launch -----------------------------------------------------------------------
// A block = R wavefronts over one tile of 64 groups: wavefront q is replica q of those groups (only wavefront q ever touches
// replica q's state), lane = group.  The tick's handlers run in the order smr_ep_cluster_tick has always fixed -- every
// replica proposes; every acceptor takes the PreAccepts senders ascending; then command leaders ascending: PreAcceptReplies,
// the Accept round where the slow path was taken, AcceptReplies, CommitNotices -- as a sequence of steps; the messages cross
// wavefronts through global arrays (the caller's out[] arrays, the reply stacks) with a block barrier where a step reads what
// another wavefront's step wrote.  Execution (durability.rs:136-160) runs behind a handler on the same lane instead of as a
// launch of its own.  115 launches of 1024 wavefronts each became one launch of 5120: the per-group work of different
// replicas overlaps, and nothing waits for a launch boundary.
template <typename T> __device__ __forceinline__ void ep_shift_ptr(T *&p, int64_t d) { p = (T *)((char *)p + d); }
__device__ __forceinline__ void ep_shift(EpView &v, int64_t d) {
    ep_shift_ptr(v.p0, d); ep_shift_ptr(v.p1, d); ep_shift_ptr(v.p2, d); ep_shift_ptr(v.p3, d); ep_shift_ptr(v.sq32, d);
    ep_shift_ptr(v.pa_seq, d); ep_shift_ptr(v.pa_deps, d); ep_shift_ptr(v.len, d); ep_shift_ptr(v.commit_bars, d);
    ep_shift_ptr(v.my_nulls, d); ep_shift_ptr(v.rewritten, d); ep_shift_ptr(v.hc, d); ep_shift_ptr(v.counters, d); ep_shift_ptr(v.xp_max, d);
    ep_shift_ptr(v.xv_status, d); ep_shift_ptr(v.xv_key, d); ep_shift_ptr(v.xv_seq, d); ep_shift_ptr(v.xv_deps, d);
}
__device__ __forceinline__ void ep_shift(EpExec &x, int64_t d) {
    ep_shift_ptr(x.exec_bars, d); ep_shift_ptr(x.prev_cb, d); ep_shift_ptr(x.digest, d);
    ep_shift_ptr(x.node_of, d); ep_shift_ptr(x.nslot, d); ep_shift_ptr(x.head, d); ep_shift_ptr(x.sib, d); ep_shift_ptr(x.parent, d);
    ep_shift_ptr(x.order, d); ep_shift_ptr(x.n_sub, d); ep_shift_ptr(x.counters, d);
}

template <int NR>
struct EpClusterArgs {
    uint32_t R, G, execute, quiet;               // quiet: handlers that can move no commit bar skip the execution pass (no recovery)
    uint32_t phase_major;                        // the leaders' steps in the order (phase, leader) instead of (leader, phase): see the kernel
    // The replicas of a cluster are created alike, so their arenas have ONE layout: replica q's arrays are replica 0's, `delta[q]`
    // bytes further on.  A wavefront builds its view from v0 / x0 with a handful of scalar adds and keeps it in SGPRs; indexing an
    // array of R views by the wavefront's number made every pointer a scalar LOAD from the kernel arguments wherever the
    // register budget had dropped it (535 per wavefront per tick, each a dependent round trip to the scalar cache).
    EpView v0;
    EpExec x0;
    int64_t delta[NR];
    uint32_t hc_slot_bytes;                      // > 0: the cluster's shared per-key table -- replica q's slot of an entry lies q * this behind replica 0's
    const uint8_t *keys[NR];
    const uint8_t *drop[NR * NR];                // [s * NR + q] (may be NULL)
    smr_ep_cluster_out out[NR];
    uint8_t *r_flags, *a_flags;                  // [s][q][G]   PreAcceptReply / AcceptReply of q to leader s
    uint64_t *r_seq;                             // [s][q][G]
    uint32_t *r_deps;                            // [s][q][R][G]
    // ep_cluster_tick_pm_kernel: the lanes whose CommitNotice phase goes one by one, for ep_cluster_commit_one_by_one_kernel --
    // defer_cnt[(parity * NR + q) * 32] lanes of replica q, their groups in defer_list[q * G ..]
    uint32_t *defer_cnt, *defer_list;
    uint32_t parity;
#ifdef EPC_STAMPS
    unsigned long long *stamps;                  // [8 blocks][NR wavefronts][64 steps]: experiments only (tools/dbg_epc_stamps.py)
#endif
};

#ifndef EPC_WAVES_PER_EU
#define EPC_WAVES_PER_EU 3                   // 168 VGPRs (147 spilled, 320 B of scratch per lane) with EPC_SETS 2: see there.  Round 3's first setting was 2
                                             // (250 VGPRs, no spills, one 5-wavefront block per CU).  Measured with per-step stamps (profiles/round3/r3r): at 168
                                             // VGPRs the hardware still ran ONE 5-wavefront block per CU; at 128 / 96 two / three blocks share a CU but each
                                             // runs 1.7-4x longer (spills + contention)
#endif
#ifndef EPC_SETS
#define EPC_SETS 2                           // sets of 64 groups per block (R <= 5): a block = EPC_SETS x R wavefronts.  Five wavefronts on a CU's four
                                             // SIMDs leave one SIMD with two of them; ten spread 3 / 3 / 2 / 2.  profiles/round3/r4i, r4k: the default order
                                             // 1078 -> 1058 us per tick, phase by phase 766 -> 711 us (the kernel is bound by instruction issue per SIMD:
                                             // two blocks' worth of wavefronts on a CU took exactly as long as one after the other)
#endif
template <int NR> constexpr int epc_sets() { return NR <= 5 ? EPC_SETS : 1; }   // (16 wavefronts of the 8-replica instance would have to fit 128 VGPRs)
// Round 4: the messages between the replica-wavefronts of a block go through LDS (NR <= 5; as rsp_cluster_tick_kernel has
// done since round 3) instead of the global reply stacks r_flags / r_seq / r_deps / a_flags and re-reads of the leaders' out[]
// arrays (the launch moved 16x its algorithmic bytes).  Lane = group in every wavefront of a set, so a
// message word is [word][lane] and its reader is the same lane of another wavefront, behind the block barrier that already
// separated the steps:
//   sh_pa  [set][leader s][10][64]: what leader s broadcasts -- word 0 flags (bit 0 proposed, bits 8-15 the decision, bit 16
//          committed), 1 col, 2 key, 3-4 seq, 5-9 deps: the PreAccept's (seq0, deps0) until s's own PreAcceptReply step
//          overwrites them with the decision's (every acceptor has taken the PreAccept by then: barrier behind step R)
//   sh_rep [set][leader s][acceptor q != s][7][64]: q's PreAcceptReply -- seq lo, seq hi, deps[5] (seq 0: no reply)
//   sh_sc  [wavefront][4][NR][64]: the lanes' per-row scalars (EpLaneT::bind_cache)
//   sh_af  [set][leader s][acceptor q][64] bytes: q's AcceptReply flag
// The out[] arrays are still WRITTEN (they are the call's outputs); nothing of the tick reads them back.  The leader's step takes
// a reply out of LDS when its turn comes instead of holding all four in registers (50 VGPRs of the old step).
template <int NR> constexpr bool epc_lds() { return NR <= 5; }
constexpr int EPC_PA_WORDS = 10, EPC_REP_WORDS = 7;       // a reply: seq lo, seq hi, deps[5]; no reply: seq 0 (a reply's seq is 1 + a max, >= 1)
template <int NR>
struct EpRepliesInLds {
    const uint32_t *rep;                                                     // sh_rep + the set's and the leader's offset
    uint32_t s, lane;
    __device__ __forceinline__ void get(uint32_t p, uint32_t &f, uint64_t &rb, uint64_t &rs, uint32_t (&rd)[NR]) const {
        const uint32_t qi = p - (p > s ? 1u : 0u);                           // (p != s: the caller skips the leader itself)
        const uint32_t *w = rep + (size_t)qi * EPC_REP_WORDS * 64 + lane;
        rs = (uint64_t)w[0] | ((uint64_t)w[64] << 32);
        f = rs != 0ull;
        rb = (f & 1u) ? (uint64_t)(s + 1u) : 0ull;                           // an acceptor replies with the message's ballot
#pragma unroll
        for (int k = 0; k < NR; k++) rd[k] = k < 5 ? w[(2 + k) * 64] : EP_NONE;
    }
};

template <int NR, bool RECOVERY>
__global__ __launch_bounds__(NR * 64 * epc_sets<NR>(), (NR <= 5 ? EPC_WAVES_PER_EU : 2)) void ep_cluster_tick_kernel(const EpClusterArgs<NR> a) {
    constexpr int SETS = epc_sets<NR>();
    constexpr bool LDS = epc_lds<NR>();
    __shared__ uint32_t sh_slow[SETS * NR];                                  // [set][leader]: some group of the set took leader s's slow path
    __shared__ uint32_t sh_pa[LDS ? SETS * NR * EPC_PA_WORDS * 64 : 1];
    __shared__ uint32_t sh_rep[LDS ? SETS * NR * (NR - 1) * EPC_REP_WORDS * 64 : 1];
    __shared__ uint8_t sh_af[LDS ? SETS * NR * NR * 64 : 1];
    __shared__ uint32_t sh_sc[SETS * NR * 4 * NR * 64];                      // the lanes' scalar caches: [wavefront][array][row][lane] (EpLaneT::bind_cache)
    const uint32_t R = a.R, G = a.G;
    const uint32_t wv = SMR_WAVE_UNIFORM(threadIdx.x >> 6), set = wv / R, q = wv - set * R;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g0 = (blockIdx.x * SETS + set) * 64u + lane;
    const bool live = g0 < G;
    const uint32_t g = live ? g0 : 0u;
    EpView v = a.v0;
    EpExec x = a.x0;
    ep_shift(v, a.delta[q]);
    ep_shift(x, a.delta[q]);
    if (a.hc_slot_bytes) v.hc = (uint32_t *)((char *)a.v0.hc + q * a.hc_slot_bytes);   // (one table for the cluster, not one per arena)
    v.me = q;
    EpLaneT<NR, true> L(v, g);
    L.bind_cache(sh_sc + (size_t)wv * 4 * NR * 64, lane);
    EpExecLaneT<NR, true> E(v, x, L, g);
    if (live) { L.load_scalars(); if (a.execute) E.load_scalars(); }
    // word w of leader s's broadcast / of acceptor qq's reply to leader s, this lane's
    auto PA = [&](uint32_t s, int w) -> uint32_t & { return sh_pa[((size_t)(set * NR + s) * EPC_PA_WORDS + w) * 64 + lane]; };
    auto RP = [&](uint32_t s, uint32_t qq, int w) -> uint32_t & {
        return sh_rep[(((size_t)(set * NR + s) * (NR - 1) + (qq - (qq > s ? 1u : 0u))) * EPC_REP_WORDS + w) * 64 + lane];
    };
    const uint32_t n_steps = 1u + R + 4u * R;
    bool slow_round = true;
#pragma unroll 1
    for (uint32_t t = 0; t < n_steps; t++) {
        bool handled = false, can_commit = false, barrier = true;
        EpInst<NR> H;                                                        // the instance this step's handler committed, if it did
        bool have_h = false;
        uint32_t h_row = 0, h_col = 0;
#ifdef EPC_STAMPS
        if ((threadIdx.x & 63u) == 0 && set == 0 && (blockIdx.x & 127u) == 5u && (blockIdx.x >> 7) < 8u)
            a.stamps[(((blockIdx.x >> 7) * NR) + q) * 64 + t] = wall_clock64();
#endif
        if (t == 0) {                                                        // every replica proposes
            if (live) {
                const smr_ep_cluster_out &o = a.out[q];
                uint8_t of; uint32_t oc; uint64_t os; uint32_t d[NR];
                const uint32_t key = a.keys[q][g];
                ep_propose_lane(L, key, 0u, of, oc, os, d);
                o.proposed[g] = of; o.col[g] = oc; o.seq0[g] = os;
#pragma unroll
                for (int i = 0; i < NR; i++) if ((uint32_t)i < R) o.deps0[(size_t)i * G + g] = d[i];
                if (LDS) {
                    PA(q, 0) = of; PA(q, 1) = oc; PA(q, 2) = key; PA(q, 3) = (uint32_t)os; PA(q, 4) = (uint32_t)(os >> 32);
#pragma unroll
                    for (int i = 0; i < NR; i++) if (i < 5) PA(q, 5 + i) = d[i];
                }
                handled = true;
            }
        } else if (t <= R) {                                                 // acceptor q: the PreAccept of sender s
            const uint32_t s = t - 1u;
            barrier = t == R;
#ifdef EPC_STAMPS
            L.sub = ((threadIdx.x & 63u) == 0 && set == 0 && (blockIdx.x & 127u) == 5u && (blockIdx.x >> 7) < 8u && t == (q == 2 ? 4u : 3u))
                        ? &a.stamps[(((blockIdx.x >> 7) * NR) + q) * 64 + 32] : nullptr;
            EPC_SUB(L, 0);
#endif
            if (s != q && live) {
                const smr_ep_cluster_out &o = a.out[s];
                const uint8_t *dm = a.drop[s * NR + q];
                uint8_t of; uint64_t ob, os; uint32_t d[NR];
                if (LDS) {
                    const bool on = (PA(s, 0) & 1u) && !(dm && dm[g]);
                    uint32_t in[NR];
#pragma unroll
                    for (int i = 0; i < NR; i++) in[i] = (i < 5 && (uint32_t)i < R) ? PA(s, 5 + i) : EP_NONE;
                    ep_acceptor_lane_in<0, NR, RECOVERY>(L, on, s, s, PA(s, 1), (uint64_t)(s + 1u), (uint64_t)PA(s, 3) | ((uint64_t)PA(s, 4) << 32), in,
                                                         PA(s, 2), of, ob, os, d);
                    const uint64_t rs = (of & 1u) ? os : 0ull;
                    RP(s, q, 0) = (uint32_t)rs; RP(s, q, 1) = (uint32_t)(rs >> 32);
#pragma unroll
                    for (int i = 0; i < NR; i++) if (i < 5) RP(s, q, 2 + i) = d[i];
                    EPC_SUB(L, 6);
                } else {
                    const bool on = (o.proposed[g] & 1) && !(dm && dm[g]);
                    ep_acceptor_lane<0, NR, RECOVERY>(L, on, s, s, o.col[g], (uint64_t)(s + 1u), o.seq0[g], o.deps0, a.keys[s][g], of, ob, os, d);
                    const size_t ro = ((size_t)s * R + q) * G + g;
                    a.r_flags[ro] = of; a.r_seq[ro] = os;
#pragma unroll
                    for (int i = 0; i < NR; i++) if ((uint32_t)i < R) a.r_deps[(((size_t)s * R + q) * R + i) * G + g] = d[i];
                }
                handled = true;
            }
        } else {
            // The command leaders' part of the tick is R x 4 steps: (leader s, phase): its PreAcceptReplies, the Accept round where
            // it went slow, its AcceptReplies, its CommitNotices.  Default order: leader by leader, as the handler-by-handler loops
            // (ep_cluster.tick, tests/ep_cluster.py) run them -- one wavefront of five works in a leader's own phases.
            // phase_major: phase by phase -- every leader's replies (all five wavefronts at once, each on its own instance), then
            // every Accept, every AcceptReply tally, every CommitNotice (an acceptor takes the senders in ascending order, as
            // before); barriers only between the phases.  A different, equally legal delivery order (the loops run it with
            // phase_major=True; the oracle cluster likewise), not bit-identical to the default one where execution is on: which
            // instances are committed at a replica when it tries to execute another one differs.
            const uint32_t u = t - 1u - R;
            const uint32_t s = a.phase_major ? u % R : u >> 2, ph = a.phase_major ? u / R : u & 3u;
            const smr_ep_cluster_out &o = a.out[s];
            if (ph == 0) {                                                   // leader s: its PreAcceptReplies, peers ascending
                if (q == s) {
                    uint8_t dec = 0;
                    if (live) {
                        uint64_t dseq; uint32_t dd[NR];
                        h_row = s;
                        if (LDS) {
                            h_col = PA(s, 1);
                            const EpRepliesInLds<NR> rdr{sh_rep + (size_t)(set * NR + s) * (NR - 1) * EPC_REP_WORDS * 64, s, lane};
                            ep_pa_replies_lane_rd<NR, true>(L, s, h_col, SMR_CTL_IDENTITY, 0u, rdr, dec, dseq, dd, &H, &have_h);
                            // the broadcast's (seq, deps) become the decision's: what the Accept / CommitNotice of s carries
                            PA(s, 0) = (PA(s, 0) & 1u) | ((uint32_t)dec << 8);
                            PA(s, 3) = dec ? (uint32_t)dseq : 0u; PA(s, 4) = dec ? (uint32_t)(dseq >> 32) : 0u;
#pragma unroll
                            for (int k = 0; k < NR; k++) if (k < 5) PA(s, 5 + k) = dec ? dd[k] : EP_NONE;
                        } else {
                            uint32_t in_f[NR]; uint64_t in_b[NR], in_s[NR]; uint32_t in_d[NR][NR];
#pragma unroll
                            for (int p = 0; p < NR; p++) {
                                const bool on = (uint32_t)p < R && (uint32_t)p != s;
                                const size_t ro = ((size_t)s * R + p) * G + g;
                                in_f[p] = on ? a.r_flags[ro] : 0u; in_s[p] = on ? a.r_seq[ro] : 0ull;
                                in_b[p] = (in_f[p] & 1u) ? (uint64_t)(s + 1u) : 0ull;   // an acceptor replies with the message's ballot
#pragma unroll
                                for (int k = 0; k < NR; k++)
                                    in_d[p][k] = (on && (uint32_t)k < R) ? a.r_deps[(((size_t)s * R + p) * R + k) * G + g] : EP_NONE;
                            }
                            h_col = o.col[g];
                            ep_pa_replies_lane(L, s, h_col, SMR_CTL_IDENTITY, 0u, in_f, in_b, in_s, in_d, dec, dseq, dd, &H, &have_h);
                        }
                        o.decision[g] = dec; o.seq[g] = dec ? dseq : 0ull;
#pragma unroll
                        for (int k = 0; k < NR; k++) if ((uint32_t)k < R) o.deps[(size_t)k * G + g] = dec ? dd[k] : EP_NONE;
                        handled = true; can_commit = true;
                    }
                    const int any_slow = __any(dec == EST_ACCEPTING);
                    if ((threadIdx.x & 63u) == 0) sh_slow[set * NR + s] = any_slow ? 1u : 0u;
                }
                if (a.phase_major) barrier = s == R - 1u;
            } else if (ph == 1) {                                            // the Accept round, where leader s took the slow path
                slow_round = sh_slow[set * NR + s] != 0;                     // (uniform over my set's wavefronts: read behind the barrier of ph 0)
                barrier = slow_round;
                for (uint32_t k = 0; k < (uint32_t)SETS; k++) barrier = barrier || sh_slow[k * NR + s] != 0;   // (the block's sets meet at the same barriers)
                if (a.phase_major) barrier = s == R - 1u;
                if (slow_round && q != s && live) {
                    uint8_t of; uint64_t ob, os; uint32_t d[NR];
                    if (LDS) {
                        uint32_t in[NR];
#pragma unroll
                        for (int i = 0; i < NR; i++) in[i] = (i < 5 && (uint32_t)i < R) ? PA(s, 5 + i) : EP_NONE;
                        ep_acceptor_lane_in<1, NR, RECOVERY>(L, ((PA(s, 0) >> 8) & 0xFFu) == EST_ACCEPTING, s, s, PA(s, 1), (uint64_t)(s + 1u),
                                                             (uint64_t)PA(s, 3) | ((uint64_t)PA(s, 4) << 32), in, PA(s, 2), of, ob, os, d);
                        sh_af[((size_t)(set * NR + s) * NR + q) * 64 + lane] = of;
                    } else {
                        ep_acceptor_lane<1, NR, RECOVERY>(L, o.decision[g] == EST_ACCEPTING, s, s, o.col[g], (uint64_t)(s + 1u), o.seq[g], o.deps,
                                                a.keys[s][g], of, ob, os, d);
                        a.a_flags[((size_t)s * R + q) * G + g] = of;
                    }
                    handled = true;
                }
            } else if (ph == 2) {                                            // leader s: the AcceptReplies, then what is committed
                if (a.phase_major) { slow_round = sh_slow[set * NR + s] != 0; barrier = s == R - 1u; }
                if (q == s && live) {
                    bool acc = false, fastc;
                    if (LDS) {
                        if (slow_round) {
                            uint32_t fm = 0;
#pragma unroll
                            for (int p = 0; p < NR; p++)
                                if ((uint32_t)p < R && (uint32_t)p != s) fm |= (uint32_t)(sh_af[((size_t)(set * NR + s) * NR + p) * 64 + lane] & 1u) << p;
                            // (a flag of an earlier tick's slow round cannot be met: a set's slow round rewrites every acceptor's flag of leader s)
                            acc = ep_accept_replies_mask(L, s, PA(s, 1), SMR_CTL_IDENTITY, fm, (uint64_t)(s + 1u));
                        }
                        fastc = ((PA(s, 0) >> 8) & 0xFFu) == EST_COMMITTED;
                        if (fastc || acc) PA(s, 0) |= 1u << 16;
                    } else {
                        acc = slow_round && ep_accept_replies_lane(L, s, o.col[g], SMR_CTL_IDENTITY, a.a_flags + (size_t)s * R * G, nullptr, (uint64_t)(s + 1u));
                        fastc = o.decision[g] == EST_COMMITTED;
                    }
                    o.committed[g] = (fastc || acc) ? 1 : 0;
                    handled = true; can_commit = true;
                }
            } else {                                                         // the CommitNotices of leader s
                barrier = false;                                             // (the next step that reads across wavefronts has its own in front)
#ifdef EPC_STAMPS
                L.sub = ((threadIdx.x & 63u) == 0 && set == 0 && (blockIdx.x & 127u) == 5u && (blockIdx.x >> 7) < 8u && s == (q == 2 ? 3u : 2u))
                            ? &a.stamps[(((blockIdx.x >> 7) * NR) + q) * 64 + 32] : nullptr;
                EPC_SUB(L, 8);
#endif
                if (q != s && live) {
                    uint8_t of; uint64_t ob, os; uint32_t d[NR];
                    h_row = s;
                    if (LDS) {
                        h_col = PA(s, 1);
                        uint32_t in[NR];
#pragma unroll
                        for (int i = 0; i < NR; i++) in[i] = (i < 5 && (uint32_t)i < R) ? PA(s, 5 + i) : EP_NONE;
                        ep_acceptor_lane_in<2, NR, RECOVERY>(L, (PA(s, 0) >> 16) & 1u, s, s, h_col, (uint64_t)(s + 1u),
                                                             (uint64_t)PA(s, 3) | ((uint64_t)PA(s, 4) << 32), in, PA(s, 2), of, ob, os, d, &H, &have_h);
                    } else {
                        h_col = o.col[g];
                        ep_acceptor_lane<2, NR, RECOVERY>(L, o.committed[g] & 1, s, s, h_col, (uint64_t)(s + 1u), o.seq[g], o.deps, a.keys[s][g], of, ob,
                                                os, d, &H, &have_h);
                    }
                    handled = true; can_commit = true;
                }
            }
        }
        EPC_SUB(L, 9);
        if (handled && a.execute && (can_commit || RECOVERY)) ep_exec_after_handler(v, x, E, have_h ? &H : nullptr, h_row, h_col);
        EPC_SUB(L, 15);
#ifdef EPC_STAMPS
        L.sub = nullptr;
#endif
        // (a barrier per set of R wavefronts, counted in LDS, so that the block's two sets drift apart and one's loads overlap the
        // other's compute: measured 2 % slower than the block barrier, profiles/r6g)
        if (barrier) __syncthreads();
    }
    if (live) { L.store_scalars(); if (a.execute) E.store_scalars(); }
#ifdef EPC_STAMPS
    if ((threadIdx.x & 63u) == 0 && set == 0 && (blockIdx.x & 127u) == 5u && (blockIdx.x >> 7) < 8u)
        a.stamps[(((blockIdx.x >> 7) * NR) + q) * 64 + n_steps] = wall_clock64();
#endif
    L.flush();
    if (a.execute) E.flush();
}

#ifdef EPC_PM_WHY
extern "C" { unsigned long long g_epc_pm_why[16]; }          /* emulator experiments only: why a lane left the batched CommitNotice phase */
#define EPC_WHY(k, cond) do { if (usual && !(cond)) atomicAdd(&g_epc_pm_why[k], 1ull); usual = usual && (cond); } while (0)
#else
#define EPC_WHY(k, cond) do { usual = usual && (cond); } while (0)
#endif
// ---- the phase-by-phase tick with a lane's handlers of one phase BATCHED (round 6) -----------------------------------------
// ep_cluster_tick_kernel in its phase-major order runs 26 steps, and a lane's 4 PreAccepts and 4 CommitNotices are 8 of them,
// each a chain of 2-4 dependent rounds of loads (profiles/r5j, s0: ~10 us a PreAccept step, 11-17 us a CommitNotice + execution
// step, of a block's ~150-200 us).  Between two barriers a lane's handlers touch that replica's state alone, so they may run
// as ONE step as long as the result is what the sequence leaves.  This kernel does that for the two long phases:
//   * the 4 PreAccepts of a lane: the 4 keys' per-key entries in one round, the <= 20 sequence numbers in a second, then the
//     four handlers back to back on registers -- what handler s would have read from memory behind handler s' < s (the
//     key's highest column in row s', the sequence number of the instance s' just stored) is patched from s' 's registers;
//   * the 4 CommitNotices of a lane with their executions: the cells' words, the keys' KV words and the digest in one round,
//     then commit + attempt_execution + the command's result of each, back to back on registers (a dependency that an earlier
//     member of the batch just executed is below that row's exec bar by then).
// Both take the common case only -- PreAccept: a fresh cell at the row's end; CommitNotice: the cell holds the PreAccepted
// instance, and execution finds every dependency executed or gone (a single-node graph, advanced_hinted's case) with no tail
// of another row waiting.  A lane outside it runs the phase's handlers one by one, as ep_cluster_tick_kernel does -- the code
// is the same (ep_acceptor_lane_in, ep_exec_after_handler), nothing of the fast path has been stored by then.
// R <= 5, no explicit prepare (a cluster with recovery keeps the step-by-step kernel).
#ifdef EPC_STAMPS
#define EPC_PM_STAMP(t) do { __builtin_amdgcn_s_waitcnt(0); if (lane == 0 && set == 0 && (blockIdx.x & 127u) == 5u && (blockIdx.x >> 7) < 8u) a.stamps[(((blockIdx.x >> 7) * NR) + q) * 64 + (t)] = wall_clock64(); } while (0)
#else
#define EPC_PM_STAMP(t) do { } while (0)
#endif
template <int NR>
__global__ __launch_bounds__(NR * 64 * epc_sets<NR>(), EPC_WAVES_PER_EU) void ep_cluster_tick_pm_kernel(const EpClusterArgs<NR> a) {
    static_assert(NR <= 5, "messages in LDS: populations <= 5");
    constexpr int SETS = epc_sets<NR>();
    __shared__ uint32_t sh_slow[SETS * NR];
    __shared__ uint32_t sh_pa[SETS * NR * EPC_PA_WORDS * 64];
    __shared__ uint32_t sh_rep[SETS * NR * (NR - 1) * EPC_REP_WORDS * 64];
    __shared__ uint8_t sh_af[SETS * NR * NR * 64];
    __shared__ uint32_t sh_sc[SETS * NR * 4 * NR * 64];
    const uint32_t R = a.R, G = a.G;
    const uint32_t wv = SMR_WAVE_UNIFORM(threadIdx.x >> 6), set = wv / R, q = wv - set * R;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g0 = (blockIdx.x * SETS + set) * 64u + lane;
    const bool live = g0 < G;
    const uint32_t g = live ? g0 : 0u;
    EpView v = a.v0;
    EpExec x = a.x0;
    ep_shift(v, a.delta[q]);
    ep_shift(x, a.delta[q]);
    if (a.hc_slot_bytes) v.hc = (uint32_t *)((char *)a.v0.hc + q * a.hc_slot_bytes);
    v.me = q;
    EpLaneT<NR, true> L(v, g);
    L.bind_cache(sh_sc + (size_t)wv * 4 * NR * 64, lane);
    EpExecLaneT<NR, true> E(v, x, L, g);
    if (live) { L.load_scalars(); if (a.execute) E.load_scalars(); }
    auto PA = [&](uint32_t s, int w) -> uint32_t & { return sh_pa[((size_t)(set * NR + s) * EPC_PA_WORDS + w) * 64 + lane]; };
    auto RP = [&](uint32_t s, uint32_t qq, int w) -> uint32_t & {
        return sh_rep[(((size_t)(set * NR + s) * (NR - 1) + (qq - (qq > s ? 1u : 0u))) * EPC_REP_WORDS + w) * 64 + lane];
    };
    const uint32_t hc_g = M24(g, v.n_keys);                                  // (entry of key k: word SHL_OF(hc_g + k, v.hc_es))
    unsigned long long n_one_by_one = 0;                                     // lanes that left a batched phase: PreAccepts (low word), CommitNotices (high)
    // The PreAccepted instance of sender s (bit s of defm) is NOT in memory yet: the record an acceptor stores for a PreAccept is its
    // reply (sequence number, dependencies: sh_rep) under the message's column and key (sh_pa), and in a running cluster the
    // CommitNotice of the same tick overwrites it -- 52 bytes written, 32 read back and up to 52 written again per (acceptor,
    // instance), and the key's entry written back a second time.  So the batched PreAccept step keeps the record (and the key's
    // highest column of row s, bit s of hcm) to itself, the batched CommitNotice step writes the cell ONCE, and whoever else
    // needs the cell in memory first -- an Accept for it, a lane that leaves a batched step, a CommitNotice that does not come
    // -- calls materialize(s): exactly the stores the PreAccept handler makes (messages.rs:60-93).  Nothing between the two
    // steps reads such a cell unasked: the leader's own handlers touch its own row, and execution looks at a dependency's cell
    // only below that row's commit bar (execution.rs:41-45), where a PreAccepting instance is not.
    uint32_t defm = 0, hcm = 0;
    auto materialize = [&](uint32_t s) {
        const uint32_t c = PA(s, 1), k = PA(s, 2);
        if (s == q) {                                                        // my own proposal: its record went out with the proposal, the key's entry waits
            if ((hcm >> s) & 1u) EA(v.hc, SHL_OF(hc_g + k, v.hc_es) + s) = c;
            hcm &= ~(1u << s);
            return;
        }
        EpInst<NR> I;
        I.make_null();
        I.bal = (uint64_t)(s + 1u);
        I.seq = (uint64_t)RP(s, q, 0) | ((uint64_t)RP(s, q, 1) << 32);
#pragma unroll
        for (int r = 0; r < NR; r++) I.d[r] = RP(s, q, 2 + r);
        I.set_status(EST_PREACCEPTING); I.set_key(k); I.set_bk(2u | (s << 2));
        L.store_inst(L.ix(s, c), I);
        if ((hcm >> s) & 1u) EA(v.hc, SHL_OF(hc_g + k, v.hc_es) + s) = c;
        defm &= ~(1u << s); hcm &= ~(1u << s);
    };
    // ... and my own proposal of this tick likewise (own_def): its record and my own PreAcceptReply go out when my PreAcceptReplies
    // step has the decision -- once, instead of a proposal's record now, 32 bytes of it read back and the decision's written then --
    // or, undecided, as the proposal left them.  Between the two only my own PreAccept handlers look at that cell (its sequence
    // number, for an instance of the same key): the batched step takes it out of sh_pa, a lane that leaves it materializes first.
    bool own_def = false;
    auto own_inst = [&]() -> EpInst<NR> {                                    // (before the PreAcceptReplies step overwrites sh_pa's seq / deps)
        EpInst<NR> I;
        I.make_null();
        I.bal = (uint64_t)(q + 1u); I.seq = (uint64_t)PA(q, 3) | ((uint64_t)PA(q, 4) << 32);
#pragma unroll
        for (int r = 0; r < NR; r++) I.d[r] = PA(q, 5 + r);
        I.set_status(EST_PREACCEPTING); I.set_key(PA(q, 2)); I.set_bk(1u); I.set_pa_acks(1u << q);
        return I;
    };
    auto materialize_own = [&]() {                                           // what ep_propose_lane stores (request.rs:48-108, durability.rs:25-35)
        if (!own_def) return;
        const EpInst<NR> I = own_inst();
        const uint32_t c = PA(q, 1);
        L.store_inst(L.ix(q, c), I);
        EA(v.pa_seq, L.ps_ix(q, c, q)) = I.seq;
        for (uint32_t r = 0; r < R; r++) EA(v.pa_deps, L.pd_ix(q, c, q, r)) = PA(q, 5 + r);
        own_def = false;
    };
    // ---- every replica proposes ----
    EPC_PM_STAMP(0);
    if (live) {
        const smr_ep_cluster_out &o = a.out[q];
        uint8_t of; uint32_t oc; uint64_t os; uint32_t d[NR];
        const uint32_t key = a.keys[q][g];
        bool up = false;
        ep_propose_lane(L, key, 0u, of, oc, os, d, &up, &own_def);
        if (up && of) hcm |= 1u << q;                                        // (my key's highest column in my row: written with the tick's other words of that line)
        o.proposed[g] = of; o.col[g] = oc; o.seq0[g] = os;
#pragma unroll
        for (int i = 0; i < NR; i++) if ((uint32_t)i < R) o.deps0[(size_t)i * G + g] = d[i];
        PA(q, 0) = of; PA(q, 1) = oc; PA(q, 2) = key; PA(q, 3) = (uint32_t)os; PA(q, 4) = (uint32_t)(os >> 32);
#pragma unroll
        for (int i = 0; i < NR; i++) PA(q, 5 + i) = d[i];
    }
    EPC_PM_STAMP(1);
    __syncthreads();
    // ---- acceptor q: the PreAccepts of every sender s != q, ascending ----
    EPC_PM_STAMP(2);
    if (live) {
        uint32_t onm = 0, col[NR], key[NR];
        bool fast = true;
#pragma unroll
        for (int s = 0; s < NR; s++) {
            col[s] = 0; key[s] = 0;
            if ((uint32_t)s >= R || (uint32_t)s == q) continue;
            const uint8_t *dm = a.drop[s * NR + q];
            col[s] = PA(s, 1); key[s] = PA(s, 2);
            if ((PA(s, 0) & 1u) && !(dm && dm[g])) {
                onm |= 1u << s;
                fast = fast && L.get_len(s) == col[s] && key[s] != EP_NO_KEY;   // a fresh cell at the row's end: nothing to pad, nothing to read of it
            } else {
                key[s] = 0;
            }
        }
        if (fast) {
            // round 1: the keys' highest columns
            // (an entry's R columns are consecutive words at an 8-byte aligned address -- a slot of R + 1 words at word q (R + 1) of the
            //  shared table's line, or a private entry of 8 / 16 words: two 8-byte loads and a word per key, not five words; every one
            //  of these is a gather over 64 lines)
            uint32_t my[NR][NR];
#pragma unroll
            for (int s = 0; s < NR; s++) {
                const bool on = (uint32_t)s < R && (uint32_t)s != q;
                const uint32_t e0 = SHL_OF(hc_g + key[s], v.hc_es);
                typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                const bool wide = on && (v.hc_es & 1u) == 0 && ((uintptr_t)v.hc & 7u) == 0;
                u32x2 a = (u32x2){EP_NONE, EP_NONE}, b = (u32x2){EP_NONE, EP_NONE};
                uint32_t c4 = EP_NONE;
                if (wide) {
                    a = *(const u32x2 *)((const char *)v.hc + (uint32_t)(e0 * 4u));
                    b = *(const u32x2 *)((const char *)v.hc + (uint32_t)(e0 * 4u + 8u));
                    c4 = EA(v.hc, e0 + 4u);
                } else if (on) {
                    a.x = EA(v.hc, e0); a.y = EA(v.hc, e0 + 1u); b.x = EA(v.hc, e0 + 2u); b.y = EA(v.hc, e0 + 3u); c4 = EA(v.hc, e0 + 4u);
                }
                my[s][0] = (on && 0u < R) ? a.x : EP_NONE;
                if (NR > 1) my[s][1 < NR ? 1 : 0] = (on && 1u < R) ? a.y : EP_NONE;
                if (NR > 2) my[s][2 < NR ? 2 : 0] = (on && 2u < R) ? b.x : EP_NONE;
                if (NR > 3) my[s][3 < NR ? 3 : 0] = (on && 3u < R) ? b.y : EP_NONE;
                if (NR > 4) my[s][4 < NR ? 4 : 0] = (on && 4u < R) ? c4 : EP_NONE;
            }
            // ... behind my own proposal, whose update of its key's entry is still with me (hcm bit q)
            if ((hcm >> q) & 1u) {
                const uint32_t cq = PA(q, 1), kq = PA(q, 2);
#pragma unroll
                for (int s = 0; s < NR; s++)
#pragma unroll
                    for (int r = 0; r < NR; r++)
                        if ((uint32_t)r == q && ((onm >> s) & 1u) && key[s] == kq && (my[s][r] == EP_NONE || cq > my[s][r])) my[s][r] = cq;
            }
            // what handler s reads behind handler s' < s of the same key: hc[key][s'] as s' left it (dependency.rs:141-167)
#pragma unroll
            for (int s = 1; s < NR; s++)
#pragma unroll
                for (int sp = 0; sp < s; sp++)
                    if (((onm >> s) & 1u) && ((onm >> sp) & 1u) && key[sp] == key[s] && (my[s][sp] == EP_NONE || col[sp] > my[s][sp])) my[s][sp] = col[sp];
            // round 2: the sequence numbers of those instances (any cell of the ring is a valid address; used only where held)
            uint64_t sq[NR][NR];
#pragma unroll
            for (int s = 0; s < NR; s++)
#pragma unroll
                for (int r = 0; r < NR; r++)
                    sq[s][r] = ((uint32_t)s < R && (uint32_t)s != q && (uint32_t)r < R) ? L.seq_at(L.ix(r, my[s][r])) : 0ull;
            uint64_t nseq[NR];
#pragma unroll
            for (int s = 0; s < NR; s++) {
                nseq[s] = 0;
                if ((uint32_t)s >= R || (uint32_t)s == q) continue;
                if (!((onm >> s) & 1u)) {                                    // not sent / lost: the empty reply
                    RP(s, q, 0) = 0u; RP(s, q, 1) = 0u;
#pragma unroll
                    for (int i = 0; i < NR; i++) RP(s, q, 2 + i) = EP_NONE;
                    continue;
                }
                const uint32_t c = col[s], k = key[s];
                L.set_len(s, c + 1u);                                        // messages.rs:33-36: the row grows by this very cell
                uint64_t ms = 0;                                             // dependency.rs:101-109
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const uint32_t d = my[s][r];
                    const bool ok = (uint32_t)r < R && d != EP_NONE && L.held((uint32_t)r < R ? r : 0, d);
                    uint64_t val = sq[s][r];
                    if (r < s && ((onm >> r) & 1u) && d == col[r]) val = nseq[r];   // the instance handler r stored an instant ago
                    if ((uint32_t)r == q && own_def && d == PA(q, 1)) val = (uint64_t)PA(q, 3) | ((uint64_t)PA(q, 4) << 32);   // my own proposal of this tick
                    if (ok && val > ms) ms = val;
                }
                ms += 1;
                uint64_t sn = (uint64_t)PA(s, 3) | ((uint64_t)PA(s, 4) << 32);
                if (ms > sn) sn = ms;
                nseq[s] = sn;
                EpInst<NR> I;
                I.make_null();
#pragma unroll
                for (int r = 0; r < NR; r++) {                               // deps.union(&my_deps), dependency.rs:85-97
                    uint32_t in = (uint32_t)r < R ? PA(s, 5 + r) : EP_NONE;
                    const uint32_t m = (uint32_t)r < R ? my[s][r] : EP_NONE;
                    if (in != EP_NONE) { if (m != EP_NONE && m > in) in = m; }
                    else in = m;
                    I.d[r] = in;
                }
                I.bal = (uint64_t)(s + 1u); I.seq = sn;
                I.set_status(EST_PREACCEPTING); I.set_key(k); I.set_bk(2u | ((uint32_t)s << 2));
                defm |= 1u << s;                                             // (the record and the key's entry: see materialize)
                if (my[s][s] == EP_NONE || c > my[s][s]) hcm |= 1u << s;
                RP(s, q, 0) = (uint32_t)sn; RP(s, q, 1) = (uint32_t)(sn >> 32);      // (sn >= 1: the reply is there)
#pragma unroll
                for (int i = 0; i < NR; i++) RP(s, q, 2 + i) = I.d[i];
            }
        } else {
            materialize(q);                                                  // (the handlers read the keys' entries in memory, and my proposal's sequence number)
            materialize_own();
            for (uint32_t s = 0; s < R; s++) {
                if (s == q) continue;
                const uint8_t *dm = a.drop[s * NR + q];
                uint8_t of; uint64_t ob, os; uint32_t d[NR];
                const bool on = (PA(s, 0) & 1u) && !(dm && dm[g]);
                uint32_t in[NR];
#pragma unroll
                for (int i = 0; i < NR; i++) in[i] = (uint32_t)i < R ? PA(s, 5 + i) : EP_NONE;
                ep_acceptor_lane_in<0, NR, false>(L, on, s, s, PA(s, 1), (uint64_t)(s + 1u), (uint64_t)PA(s, 3) | ((uint64_t)PA(s, 4) << 32), in,
                                                  PA(s, 2), of, ob, os, d);
                const uint64_t rs = (of & 1u) ? os : 0ull;
                RP(s, q, 0) = (uint32_t)rs; RP(s, q, 1) = (uint32_t)(rs >> 32);
#pragma unroll
                for (int i = 0; i < NR; i++) RP(s, q, 2 + i) = d[i];
            }
            n_one_by_one += 1ull;                                            // (smr_ep_cluster_batch_stats)
        }
    }
    EPC_PM_STAMP(3);
    __syncthreads();
    // ---- command leader q: its PreAcceptReplies, peers ascending (messages.rs:96-270), and the execution behind a fast commit ----
    EPC_PM_STAMP(4);
    {
        uint8_t dec = 0;
        if (live) {
            const smr_ep_cluster_out &o = a.out[q];
            uint64_t dseq; uint32_t dd[NR];
            EpInst<NR> H;
            bool have_h = false;
            const uint32_t h_col = PA(q, 1);
            const EpRepliesInLds<NR> rdr{sh_rep + (size_t)(set * NR + q) * (NR - 1) * EPC_REP_WORDS * 64, q, lane};
            const EpInst<NR> mine = own_inst();
            ep_pa_replies_lane_rd<NR, true>(L, q, h_col, SMR_CTL_IDENTITY, 0u, rdr, dec, dseq, dd, &H, &have_h, &mine, own_def);
            own_def = false;                                                 // (decided or not, the cell is in memory now)
            PA(q, 0) = (PA(q, 0) & 1u) | ((uint32_t)dec << 8);
            PA(q, 3) = dec ? (uint32_t)dseq : 0u; PA(q, 4) = dec ? (uint32_t)(dseq >> 32) : 0u;
#pragma unroll
            for (int k = 0; k < NR; k++) PA(q, 5 + k) = dec ? dd[k] : EP_NONE;
            o.decision[g] = dec; o.seq[g] = dec ? dseq : 0ull;
#pragma unroll
            for (int k = 0; k < NR; k++) if ((uint32_t)k < R) o.deps[(size_t)k * G + g] = dec ? dd[k] : EP_NONE;
            if (a.execute) ep_exec_after_handler(v, x, E, have_h ? &H : nullptr, q, h_col);
        }
        const int any_slow = __any(dec == EST_ACCEPTING);
        if (lane == 0) sh_slow[set * NR + q] = any_slow ? 1u : 0u;
    }
    EPC_PM_STAMP(5);
    __syncthreads();
    EPC_PM_STAMP(6);
    // ---- the Accept round of every leader that took the slow path in some group of my set (messages.rs:273-345) ----
    {
        bool any = false;
        for (uint32_t k = 0; k < (uint32_t)SETS * R; k++) any = any || sh_slow[k] != 0;
        if (any) {                                                           // (block-uniform: the barrier below is met by all or none)
            for (uint32_t s = 0; s < R; s++) {
                if (sh_slow[set * NR + s] == 0 || s == q || !live) continue;
                uint8_t of; uint64_t ob, os; uint32_t d[NR], in[NR];
#pragma unroll
                for (int i = 0; i < NR; i++) in[i] = (uint32_t)i < R ? PA(s, 5 + i) : EP_NONE;
                if (((PA(s, 0) >> 8) & 0xFFu) == EST_ACCEPTING && ((defm >> s) & 1u)) materialize(s);   // (the handler reads the cell)
                ep_acceptor_lane_in<1, NR, false>(L, ((PA(s, 0) >> 8) & 0xFFu) == EST_ACCEPTING, s, s, PA(s, 1), (uint64_t)(s + 1u),
                                                  (uint64_t)PA(s, 3) | ((uint64_t)PA(s, 4) << 32), in, PA(s, 2), of, ob, os, d);
                sh_af[((size_t)(set * NR + s) * NR + q) * 64 + lane] = of;
            }
            __syncthreads();
        }
    }
    // ---- command leader q: the AcceptReplies (messages.rs:348-436), then what is committed ----
    EPC_PM_STAMP(7);
    if (live) {
        const smr_ep_cluster_out &o = a.out[q];
        bool acc = false;
        if (sh_slow[set * NR + q] != 0) {
            uint32_t fm = 0;
#pragma unroll
            for (int p = 0; p < NR; p++)
                if ((uint32_t)p < R && (uint32_t)p != q) fm |= (uint32_t)(sh_af[((size_t)(set * NR + q) * NR + p) * 64 + lane] & 1u) << p;
            acc = ep_accept_replies_mask(L, q, PA(q, 1), SMR_CTL_IDENTITY, fm, (uint64_t)(q + 1u));
        }
        const bool fastc = ((PA(q, 0) >> 8) & 0xFFu) == EST_COMMITTED;
        if (fastc || acc) PA(q, 0) |= 1u << 16;
        o.committed[g] = (fastc || acc) ? 1 : 0;
        if (a.execute) ep_exec_after_handler(v, x, E);
    }
    EPC_PM_STAMP(8);
    __syncthreads();
    EPC_PM_STAMP(9);
    // ---- acceptor q: the CommitNotices of every leader s != q, ascending (messages.rs:438-508), each with its execution ----
    bool defer = false;
    if (live) {
        const uint32_t W = v.W;
        // every instance of this tick by its row r: (r, col[r]) with key[r] and -- in LDS, the leader's broadcast -- the decision's
        // seq / deps; onm: the CommitNotices I take; my own row's instance matters where its execution is still waiting (below)
        uint32_t onm = 0, col[NR], key[NR];
        bool usual = true;
        EPC_WHY(0, !L.rewritten);
        uint32_t s_last = 0;                                                 // the phase's last handler: what smr_ep_exec_poll reports
#pragma unroll
        for (int s = 0; s < NR; s++) {
            col[s] = 0; key[s] = 0;
            if ((uint32_t)s >= R) continue;
            const bool committed = (PA(s, 0) >> 16) & 1u;
            if (committed) { col[s] = PA(s, 1); key[s] = PA(s, 2); }
            if ((uint32_t)s == q) continue;
            s_last = s;
            if (committed) { onm |= 1u << s; EPC_WHY(1, key[s] != EP_NO_KEY); }
        }
        if (key[0] == EP_NO_KEY) key[0] = 0;                                 // (a clamped key for the loads; such a lane has left the fast path)
#pragma unroll
        for (int s = 1; s < NR; s++) if (key[s] == EP_NO_KEY) key[s] = 0;
        // the one round of loads: the cells' ballot / sequence and meta words, the keys' KV words, the digest
        u32x4 w0[NR], w2[NR]; uint32_t kvcur[NR];
#pragma unroll
        for (int s = 0; s < NR; s++) {
            const bool m = (uint32_t)s < R;
            const uint32_t i = L.ix(m ? s : 0u, col[s]);
            w0[s] = (u32x4){0u, 0u, 0u, 0u}; w2[s] = (u32x4){0u, 0u, 0u, 0u};
            if ((defm >> s) & 1u) {                                          // what materialize(s) would have stored: known, not loaded
                w0[s] = (u32x4){(uint32_t)(s + 1u), 0u, RP(s, q, 0), RP(s, q, 1)};
                w2[s] = (u32x4){RP(s, q, 6), (uint32_t)EST_PREACCEPTING | (PA(s, 2) << 8) | ((2u | ((uint32_t)s << 2)) << 16), 0u, EP_NONE};
            } else if (m) {
                if ((uint32_t)s != q) w0[s] = EA(v.p0, i);
                w2[s] = EA(v.p2, i);
            }
            kvcur[s] = (m && a.execute) ? EA(v.hc, SHL_OF(hc_g + key[s], v.hc_es) + v.hc_kv) : 0u;
        }
        uint64_t dg = a.execute ? EA(x.digest, g) : 0ull;
        // the scalars the members move, on copies: commit bars, exec bars (row lengths stay)
        uint32_t cbL[NR], ebL[NR];
        // pend: rows whose tail is THIS tick's instance, Committed and waiting for its execution (attempt_execution abandoned:
        // a dependency was not committed here yet) -- what the re-attempts behind a successful attempt go through
        // (durability.rs:148-158).  Going in, that can only be my own row (my instance committed a phase ago).
        uint32_t pend = 0;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            cbL[r] = (uint32_t)r < R ? L.get_cb(r) : 0u;
            ebL[r] = ((uint32_t)r < R && a.execute) ? E.get_eb(r) : 0u;
            if ((uint32_t)r < R && a.execute) {
                EPC_WHY(2, L.cw(3, r) == cbL[r]);                            // (no commit bar moved unseen: cb_moved would say so)
                if (cbL[r] != ebL[r]) {
                    const bool mine = (uint32_t)r == q && ((PA(r, 0) >> 16) & 1u) && cbL[r] == ebL[r] + 1u && ebL[r] == col[r] &&
                                      L.get_len(r) == cbL[r] && (w2[r].y & 0xFFu) == EST_COMMITTED && ((w2[r].y >> 8) & 0xFFu) == key[r] &&
                                      PA(r, 2) != EP_NO_KEY;
                    EPC_WHY(8, mine);
                    pend |= 1u << r;
                }
            }
        }
        uint32_t stf[NR];                                                    // per row: the final Status of this tick's instance where this phase sets it (0: untouched)
        uint32_t n_exec = 0, n_att = 0, n_unh = 0, n_abort = 0, last_sub = 0;
        uint64_t ord_lo = 0, ord_hi = 0; uint32_t ordm = 0;                  // the submission list as the phase leaves it: position k written (bit k), 16 bits each
                                                                             // (an array here became a runtime-indexed one in scratch: `if (n == k) a[k] = x` for every k is a[n] = x to the compiler)
        uint32_t exm = 0;                                                    // rows whose instance was executed in this phase
#pragma unroll
        for (int r = 0; r < NR; r++) stf[r] = 0;
        // attempt_execution (execution.rs:25-149) from the tail (r, col[r]) as far as this path goes: every dependency and the row
        // predecessor not committed here (abandoned), gone from the ring, or Executed / Executing -- below its row's exec bar as
        // moved so far; anything else (a second node of the graph) leaves the fast path.  true = the instance may run.
        auto attempt = [&](auto RC) -> bool {
            constexpr int r = decltype(RC)::value;
            bool abandoned = false;
            uint32_t unheld = 0;
#pragma unroll
            for (int e = 0; e <= NR; e++) {
                const uint32_t d = e < NR ? ((uint32_t)e < R ? PA(r, 5 + (e < NR ? e : 0)) : EP_NONE) : (col[r] > 0 ? col[r] - 1u : EP_NONE);
                constexpr int er_c = 0;
                (void)er_c;
                const int er = e < NR ? e : r;
                if (d == EP_NONE || abandoned) continue;
                if (d >= cbL[er]) { abandoned = true; continue; }            // execution.rs:41-45
                if (!L.held(er, d)) { unheld++; continue; }                  // (left the ring = executed)
#ifdef EPC_PM_WHY
                if (usual && !(d < ebL[er])) printf("why9 g=%u q=%u r=%d e=%d d=%u col=[%u %u %u %u %u] key=[%u %u %u %u %u] onm=%x pend=%x exm=%x cb=[%u %u %u %u %u] eb=[%u %u %u %u %u] deps_r=[%d %d %d %d %d] deps_er=[%d %d %d %d %d]\n", g, q, r, e, d, col[0], col[1], col[2], col[3], col[4], key[0], key[1], key[2], key[3], key[4], onm, pend, exm, cbL[0], cbL[1], cbL[2], cbL[3], cbL[4], ebL[0], ebL[1], ebL[2], ebL[3], ebL[4], (int)PA(r,5), (int)PA(r,6), (int)PA(r,7), (int)PA(r,8), (int)PA(r,9), (int)PA(er < NR ? er : 0,5), (int)PA(er < NR ? er : 0,6), (int)PA(er < NR ? er : 0,7), (int)PA(er < NR ? er : 0,8), (int)PA(er < NR ? er : 0,9));
#endif
                EPC_WHY(9 + (e == NR ? 1 : 0), d < ebL[er]);                 // below the exec bar: Executed (or Executing: an earlier member of this very handler)
            }
            n_att++; n_unh += unheld;
            if (abandoned) n_abort++;
            return !abandoned;
        };
        // execution.rs:105-142 + the command's result (:152-211) for the single-node graph (r, col[r]); n_ord: position in the handler's list
        auto run = [&](auto RC, uint32_t &n_ord) {
            constexpr int r = decltype(RC)::value;
            const uint64_t tok = ((uint64_t)(r + 1u) << 32) | col[r];
            const uint64_t old = ep_kv_unpack(kvcur[r]);
            EPC_WHY(13, col[r] < EP_KV_COL_LIMIT);                           // (counted where the handlers run one by one)
            dg = (dg ^ tok) * EP_DG_MUL; dg = (dg ^ old) * EP_DG_MUL;
            const uint32_t tw = ep_kv_pack(tok);
#pragma unroll
            for (int r2 = 0; r2 < NR; r2++) if (key[r2] == key[r]) kvcur[r2] = tw;   // (the key's KV word as every later reader of it sees it)
            const uint32_t ring = ((uint32_t)r << E.wshift) | (col[r] & v.Wmask);
            if (n_ord < (uint32_t)NR) {
                const uint64_t sh = (uint64_t)(ring & 0xFFFFu) << (16u * (n_ord & 3u));
                if (n_ord < 4u) ord_lo |= sh; else ord_hi |= sh;
                ordm |= 1u << n_ord;
            }
            EPC_WHY(11, n_ord < (uint32_t)NR);
            n_ord++;
            exm |= 1u << r; n_exec++;
            stf[r] = EST_EXECUTED;
            if (col[r] == ebL[r]) ebL[r] = col[r] + 1u;
            pend &= ~(1u << r);
        };
        auto member = [&](auto SC) {
            constexpr int s = decltype(SC)::value;
            if (!((onm >> s) & 1u)) return;
            const uint32_t c = col[s], k = key[s], len = L.get_len(s);
            const uint64_t bal = (uint64_t)w0[s].x | ((uint64_t)w0[s].y << 32);
            const uint32_t m0 = w2[s].y;
            EPC_WHY(3, c < len && c + W >= len);                             // the cell is in the ring
            EPC_WHY(4, (uint64_t)(s + 1u) >= bal);                           // messages.rs:455
            EPC_WHY(5, (m0 & 0xFFu) != EST_NULL && ((m0 >> 8) & 0xFFu) == k);   // it holds this instance (its PreAccept came by): the key's entry stands
            EPC_WHY(6, c >= cbL[s]);                                         // not a rewrite below the commit bar
            stf[s] = EST_COMMITTED;
            if (c != cbL[s]) return;                                         // (a gap below it: the bar stays)
            EPC_WHY(7, len == c + 1u);                                       // durability.rs:104-135: the bar moves over this cell -- and no further
            cbL[s] = c + 1u;
            if (!a.execute) return;
            EPC_WHY(12, c == ebL[s]);                                        // durability.rs:136-160 -> execution.rs:25-149 from the tail (s, c)
            uint32_t n_ord = 0;
            if (attempt(SC)) {
                run(SC, n_ord);
                // the re-attempts on every OTHER row whose tail is still Committed, rows ascending, found before any of them runs
                const uint32_t re = pend & ~(1u << s);
                auto again = [&](auto RC) {
                    constexpr int r = decltype(RC)::value;
                    if (r != s && ((re >> r) & 1u) && attempt(RC)) run(RC, n_ord);
                };
                again(std::integral_constant<int, 0>{}); again(std::integral_constant<int, 1>{}); again(std::integral_constant<int, 2>{});
                again(std::integral_constant<int, 3>{}); again(std::integral_constant<int, 4>{});
            } else {
                pend |= 1u << s;
            }
            if ((uint32_t)s == s_last) last_sub = n_ord;
        };
        member(std::integral_constant<int, 0>{}); member(std::integral_constant<int, 1>{}); member(std::integral_constant<int, 2>{});
        member(std::integral_constant<int, 3>{}); member(std::integral_constant<int, 4>{});
        if (usual) {
#pragma unroll
            for (int s = 0; s < NR; s++) {
                if ((uint32_t)s >= R || !stf[s]) continue;
                const uint32_t c = col[s], i = L.ix(s, c);
                if ((uint32_t)s != q) {
                    const uint32_t sl = PA(s, 3), sh = PA(s, 4);
                    const bool fresh = (defm >> s) & 1u;                     // nothing of the cell is in memory: every word goes out, once
                    if (fresh && ((hcm >> s) & 1u)) EA(v.hc, SHL_OF(hc_g + key[s], v.hc_es) + s) = c;
                    defm &= ~(1u << s); hcm &= ~(1u << s);
                    if (fresh || w0[s].x != (uint32_t)(s + 1u) || w0[s].y != 0u || w0[s].z != sl || w0[s].w != sh) {
                        EA(v.p0, i) = (u32x4){(uint32_t)(s + 1u), 0u, sl, sh};
                        EA(v.sq32, i) = (sh == 0u && sl != 0xFFFFFFFFu) ? sl : 0xFFFFFFFFu;
                    }
                    // deps[0..3] as my PreAcceptReply of this tick carried them are what the cell holds while it is still PreAccepting:
                    // the word is written only where the decision differs
                    const bool same_p1 = !fresh && (w2[s].y & 0xFFu) == EST_PREACCEPTING && (RP(s, q, 0) | RP(s, q, 1)) != 0u && RP(s, q, 2) == PA(s, 5) && RP(s, q, 3) == PA(s, 6) &&
                                         RP(s, q, 4) == PA(s, 7) && RP(s, q, 5) == PA(s, 8);
                    if (!same_p1)
                        EA(v.p1, i) = (u32x4){PA(s, 5), NR > 1 ? PA(s, 6) : EP_NONE, NR > 2 ? PA(s, 7) : EP_NONE, NR > 3 ? PA(s, 8) : EP_NONE};
                    EA(v.p2, i) = (u32x4){NR > 4 ? PA(s, 9) : EP_NONE, (w2[s].y & 0xFFFF0000u) | (key[s] << 8) | stf[s], w2[s].z, EP_NONE};
                } else {
                    EA(v.p2, i) = (u32x4){w2[s].x, (w2[s].y & ~0xFFu) | stf[s], w2[s].z, w2[s].w};   // (my own instance ran behind a member: its Status alone)
                }
                if ((exm >> s) & 1u) EA(v.hc, SHL_OF(hc_g + key[s], v.hc_es) + v.hc_kv) = kvcur[s];
            }
#pragma unroll
            for (int r = 0; r < NR; r++) {
                if ((uint32_t)r >= R) continue;
                L.set_cb(r, cbL[r]);
                if (a.execute) { E.set_eb(r, ebL[r]); L.cw(3, r) = cbL[r]; }
            }
            if (a.execute) {
                if (exm) EA(x.digest, g) = dg;
#pragma unroll
                for (int k = 0; k < NR; k++) if ((ordm >> k) & 1u) EA(x.order, E.at(k)) = (uint16_t)((k < 4 ? ord_lo : ord_hi) >> (16 * (k & 3)));
                EA(x.n_sub, g) = last_sub;
                E.c_exec += n_exec; E.c_attempts += n_att; E.c_unheld += n_unh; E.c_aborts += n_abort;
            }
            for (uint32_t s = 0; s < R; s++)                                 // a PreAccepted instance whose CommitNotice did not come: as the handler leaves it
                if (((defm | hcm) >> s) & 1u) materialize(s);                //     (and my own key's entry)
        } else {
            for (uint32_t s = 0; s < R; s++) if (((defm | hcm) >> s) & 1u) materialize(s);
            defer = true;                                                    // nothing of this phase has been stored for the lane
            n_one_by_one += 1ull << 32;
        }
    }
    {   // the lanes that go one by one: onto replica q's list (one atomic per wavefront)
        const unsigned long long dm = __ballot(defer);
        if (dm) {
            const uint32_t first = (uint32_t)__ffsll(dm) - 1u;
            uint32_t base = 0;
            if (lane == first) base = atomicAdd(&a.defer_cnt[(a.parity * NR + q) * 32u], (uint32_t)__popcll(dm));
            base = __shfl(base, (int)first);
            if (defer) a.defer_list[(size_t)q * G + base + (uint32_t)__popcll(dm & ((1ull << lane) - 1ull))] = g;
        }
    }
    EPC_PM_STAMP(10);
    if (live) { L.store_scalars(); if (a.execute) E.store_scalars(); }
    EPC_PM_STAMP(11);
    L.flush();
    if (a.execute) E.flush();
    for (int off = 32; off > 0; off >>= 1) n_one_by_one += __shfl_xor(n_one_by_one, off);
    if (lane == 0 && n_one_by_one) ctr_add(v.counters, 7, n_one_by_one);
}

// The CommitNotice phase of the lanes ep_cluster_tick_pm_kernel put on its lists (a Commit for a cell that does not hold the
// PreAccepted instance, an execution whose graph has a second node, ...: under 1 % of the lanes of a running cluster, but one per
// wavefront there would hold its whole block for four handlers' round trips): handler by handler, the messages out of the
// tick's output arrays, a wavefront of listed lanes per block (blockIdx.x = the replica, so that the blocks with work -- the first
// n / EPC_CL_LANES of every replica -- are the first the dispatcher places: with the replica as blockIdx.y the last replica's chains started
// behind four replicas' rows of empty blocks).  Also empties the OTHER parity's
// counts for the next tick.
#ifndef EPC_CL_LANES
#define EPC_CL_LANES 2u                       // (1: the same; 4: +12 us per tick, 8: +6, profiles/s28)
#endif
#ifndef EPC_CL_MAX_BLOCKS                     // the grid's blocks per replica: a longer list walks the loop below in several passes
#define EPC_CL_MAX_BLOCKS 1024u               // (the emulator builds with a small cap so that its tests take those passes)
#endif
#ifdef EPC_CL_NOLDS                                 // (experiments, profiles/s35: the launch without LDS -- per-row scalars and the walk's arrays in place -- so that
constexpr bool EPC_CL_LDS = false;                  //  its blocks fit on a CU beside a block of the batched kernel)
#else
constexpr bool EPC_CL_LDS = true;
#endif
template <int NR>
__global__ __launch_bounds__(64) void ep_cluster_commit_one_by_one_kernel(const EpClusterArgs<NR> a) {
    __shared__ uint32_t sh_sc[EPC_CL_LDS ? 4 * NR * 64 : 1];
    constexpr uint32_t WALK_CELLS = EPC_CL_LDS ? 512 : 0;                    // population * window up to here: the walk's arrays in LDS
    __shared__ uint16_t sh_walk[EPC_CL_LDS ? 7 * WALK_CELLS * EPC_CL_LANES : 1];   // node_of, nslot, head, sib, parent [cell][lane]; order [2 cells][lane]
    const uint32_t q = blockIdx.x, bx = blockIdx.y, nbx = gridDim.y, R = a.R, G = a.G, lane = threadIdx.x;
    const uint32_t n = SMR_WAVE_UNIFORM(a.defer_cnt[(a.parity * NR + q) * 32u]);
    if (bx != 0u && bx * EPC_CL_LANES >= n) return;                           // (block 0 also empties the other parity's count, below)
    const uint32_t RW = R * a.v0.W;
    const bool lds_walk = a.execute && RW <= WALK_CELLS;
    if (lds_walk) for (uint32_t i = lane; i < RW * EPC_CL_LANES; i += 64u) sh_walk[i] = 0;   // node_of: zero between attempts (the walk leaves it so)
    __syncthreads();
    if (bx == 0 && lane == 0) a.defer_cnt[((a.parity ^ 1u) * NR + q) * 32u] = 0;
    EpView v = a.v0;
    EpExec x = a.x0;
    ep_shift(v, a.delta[q]);
    ep_shift(x, a.delta[q]);
    if (a.hc_slot_bytes) v.hc = (uint32_t *)((char *)a.v0.hc + q * a.hc_slot_bytes);
    v.me = q;
    // EPC_CL_LANES listed lanes per wavefront, not 64: the walks of attempt_execution are chains of ~30 dependent round trips that
    // different lanes enter behind different members of the batch, and a wavefront pays every one of them in turn (64 lanes
    // per wavefront: 250 us for ~2 750 listed lanes, profiles/s6: the fourth member's step alone 100 us)
    for (uint32_t base = bx * EPC_CL_LANES; base < n; base += nbx * EPC_CL_LANES) {
        const bool active = lane < EPC_CL_LANES && base + lane < n;
        const uint32_t g = active ? a.defer_list[(size_t)q * G + base + lane] : 0u;
        EpLaneT<NR, EPC_CL_LDS> L(v, g);                                    // (the lane's per-row scalars in LDS, as in the tick kernel: every handler starts with them)
        if (EPC_CL_LDS) L.bind_cache(sh_sc, lane);
        EpExec xl = x;
        if (lds_walk) {
            xl.node_of = sh_walk; xl.nslot = sh_walk + RW * EPC_CL_LANES; xl.head = sh_walk + 2 * RW * EPC_CL_LANES;
            xl.sib = sh_walk + 3 * RW * EPC_CL_LANES; xl.parent = sh_walk + 4 * RW * EPC_CL_LANES; xl.order = sh_walk + 5 * RW * EPC_CL_LANES;
        }
        EpExecLaneT<NR, EPC_CL_LDS> E(v, xl, L, g);
        if (lds_walk) E.walk_in(EPC_CL_LANES, lane < EPC_CL_LANES ? lane : 0u);
        uint32_t n_listed = 0;                                               // (the longest submission list a handler of this lane left)
        if (active) { L.load_scalars(); if (a.execute) E.load_scalars(); }
#ifdef EPC_STAMPS
#define EPC_CL_STAMP(k) do { __builtin_amdgcn_s_waitcnt(0); if (lane == 0 && bx == 0 && base == 0) a.stamps[q * 64 + 40 + (k)] = wall_clock64(); } while (0)
#else
#define EPC_CL_STAMP(k) do { } while (0)
#endif
        EPC_CL_STAMP(0);
        if (active)
            for (uint32_t s = 0; s < R; s++) {
                if (s == q) continue;
                const smr_ep_cluster_out &o = a.out[s];
                uint8_t of; uint64_t ob, os; uint32_t d[NR];
                EpInst<NR> H;
                bool have_h = false;
                const uint32_t h_col = o.col[g];
                ep_acceptor_lane<2, NR, false>(L, o.committed[g] & 1, s, s, h_col, (uint64_t)(s + 1u), o.seq[g], o.deps, a.keys[s][g], of, ob, os, d, &H, &have_h);
                EPC_CL_STAMP(1 + 2 * s);
                if (a.execute) { ep_exec_after_handler(v, xl, E, have_h ? &H : nullptr, s, h_col); n_listed = E.n_order > n_listed ? E.n_order : n_listed; }
                EPC_CL_STAMP(2 + 2 * s);
            }
        if (active && lds_walk)                                              // the lists as the handlers left them, where smr_ep_exec_poll reads them
            for (uint32_t k = 0; k < n_listed; k++) EA(x.order, M24(k, G) + g) = xl.order[k * EPC_CL_LANES + lane];
        if (active) { L.store_scalars(); if (a.execute) E.store_scalars(); }
        EPC_CL_STAMP(11);
        L.flush();
        if (a.execute) E.flush();
    }
}
}  // namespace smr

extern "C" {

int smr_ep_replica_create(const smr_ep_cfg *cfg, smr_ep_replica **out) {
    if (!cfg || !out) return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (cfg->n_groups == 0) return fail(SMR_ERR_ARG, "epaxos: n_groups is zero");
    if (cfg->population < 3 || cfg->population > SMR_MAX_REPLICAS) return fail(SMR_ERR_ARG, "epaxos: population must be in 3..8");
    if (cfg->me >= cfg->population) return fail(SMR_ERR_ARG, "epaxos: replica id out of range");
    if (!cfg->window || (cfg->window & (cfg->window - 1)) || cfg->window < 8)
        return fail(SMR_ERR_ARG, "epaxos: window must be a power of two >= 8");
    if (cfg->n_keys == 0 || cfg->n_keys > 255) return fail(SMR_ERR_ARG, "epaxos: n_keys must be in 1..255");
    if (cfg->execute > 1) return fail(SMR_ERR_ARG, "epaxos: execute must be 0 or 1");
    if (cfg->recovery > 1) return fail(SMR_ERR_ARG, "epaxos: recovery must be 0 or 1");
    if (cfg->execute && (uint64_t)cfg->population * cfg->window > 32768)
        return fail(SMR_ERR_ARG, "epaxos: execution keeps 15-bit ring cell ids: population * window must be <= 32768");
    {   // every array is addressed through 32-bit byte offsets (EA): the largest must stay under 4 GB
        const uint64_t G = cfg->n_groups, W = cfg->window, R = cfg->population, K = cfg->n_keys, PR = cfg->recovery ? R : 1;
        uint64_t most = R * W * G * 16;                                          // a record plane
        most = std::max(most, PR * W * R * R * G * 4);                           // pa_deps / xv_deps
        most = std::max(most, K * (R <= 6 ? 8 : 16) * G * 4);                   // hc (with the KV words)
        if (most >= (1ull << 32))
            return fail(SMR_ERR_ARG, "epaxos: n_groups * window too large: an array would pass 4 GB (32-bit offsets); shard the groups over more replicas objects");
        if (W * R * R * PR >= (1ull << 24) || G >= (1ull << 24))                 // (M24: the index arithmetic's 24-bit multiplies)
            return fail(SMR_ERR_ARG, "epaxos: window * population^2 (* population with recovery) and n_groups must stay below 2^24 (24-bit index arithmetic)");
    }
    smr_ep_replica *e = new smr_ep_replica();
    e->cfg = *cfg;
    memset(&e->v, 0, sizeof(e->v));
    memset(&e->x, 0, sizeof(e->x));
    ep_layout(e, true);
    e->arena.size = e->arena.used + 256;
    hipError_t err = hipMalloc((void **)&e->arena.base, e->arena.size);
    if (err != hipSuccess) { delete e; return fail(SMR_ERR_DEVICE, std::string("epaxos: hipMalloc: ") + hipGetErrorString(err)); }
    ep_layout(e, false);
    EpView &v = e->v;
    const uint32_t R = cfg->population;
    v.G = cfg->n_groups; v.W = cfg->window; v.Wmask = cfg->window - 1; v.R = R; v.me = cfg->me; v.n_keys = cfg->n_keys;
    v.recovery = cfg->recovery;
    v.hc_ew = R <= 6 ? 8u : 16u;
    v.hc_es = v.hc_ew; v.hc_kv = v.hc_ew - 2u;
    v.simple_q = R / 2 + 1;                                                      // mod.rs:693
    v.super_q = cfg->optimized_quorum ? R / 2 + (R / 2 + 1) / 2 : (R / 2) * 2;   // mod.rs:694-698
    err = hipMemset(e->arena.base, 0, e->arena.size);
    if (err == hipSuccess) err = hipMemset(v.hc, 0xFF, (size_t)cfg->n_keys * v.hc_ew * v.G * 4);
    if (err == hipSuccess)                                                       // ... and every entry's KV word 0
        err = hipMemset2D((char *)v.hc + v.hc_kv * 4, (size_t)v.hc_es * 4, 0, 8, (size_t)cfg->n_keys * v.G);
    if (err == hipSuccess) {                                                     // every ring cell a null instance (deps None, key None)
        const size_t n = (size_t)R * v.W * v.G;
        hipLaunchKernelGGL(ep_init_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)nullptr, v.p1, v.p2, v.p3, n);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    if (err == hipSuccess) err = hipMalloc((void **)&e->wire_acc, EW_ACC_WORDS * 8);
    if (err == hipSuccess) err = hipMemset(e->wire_acc, 0, EW_ACC_WORDS * 8);
    if (err != hipSuccess) {
        if (e->wire_acc) (void)hipFree(e->wire_acc);
        (void)hipFree(e->arena.base); delete e;
        return fail(SMR_ERR_DEVICE, std::string("epaxos: init: ") + hipGetErrorString(err));
    }
    *out = e;
    return SMR_OK;
}

void smr_ep_replica_destroy(smr_ep_replica *e) {
    if (!e) return;
    if (e->seat) *e->seat = nullptr;                             // (the cluster then has nothing of mine to hand back)
    if (e->arena.base) (void)hipFree(e->arena.base);
    if (e->wire_acc) (void)hipFree(e->wire_acc);
    snap_glist_free(e->glist);
    delete e;
}

#define EP_GRID(e) dim3(((e)->v.G + 255) / 256), dim3(256), 0, (hipStream_t)stream

// the attempts of handle_logged_commit_slot for whatever the kernel just launched committed
static int ep_execute(smr_ep_replica *e, void *stream) {
    if (!e->cfg.execute || e->skip_exec) return SMR_OK;
    if (e->v.R <= 5) hipLaunchKernelGGL(ep_execute_kernel<5>, EP_GRID(e), e->v, e->x);
    else hipLaunchKernelGGL(ep_execute_kernel<EMAXR>, EP_GRID(e), e->v, e->x);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_ep_propose(smr_ep_replica *e, const uint8_t *key_dev, const uint8_t *exploded_dev, const smr_ep_msg *out,
                   void *stream) {
    if (!e || !key_dev || !out || !out->flags || !out->col || !out->seq || !out->deps)
        return fail(SMR_ERR_ARG, "epaxos: null argument");
    hipLaunchKernelGGL(ep_propose_kernel, EP_GRID(e), e->v, key_dev, exploded_dev, out->flags, out->col, out->seq, out->deps);
    SMR_HIP_TRY(hipGetLastError());
    return ep_execute(e, stream);
}

static int ep_acceptor(smr_ep_replica *e, int mode, const smr_ep_msg *m, const smr_ep_msg *r, void *stream) {
    if (!e || !m || !m->flags || !m->peer || !m->col || !m->ballot || !m->seq || !m->deps || !m->key)
        return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (mode != 2 && (!r || !r->flags || !r->ballot || (mode == 0 && (!r->seq || !r->deps))))
        return fail(SMR_ERR_ARG, "epaxos: null reply buffers");
    if (m->row && !e->cfg.recovery) return fail(SMR_ERR_STATE, "epaxos: a message with a row of its own needs smr_ep_cfg.recovery");
    if (mode == 2)
        hipLaunchKernelGGL(ep_acceptor_kernel<2>, EP_GRID(e), e->v, m->flags, m->peer, m->col, m->ballot, m->seq, m->deps,
                           m->key, (uint8_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, m->row);
    else if (mode == 1)
        hipLaunchKernelGGL(ep_acceptor_kernel<1>, EP_GRID(e), e->v, m->flags, m->peer, m->col, m->ballot, m->seq, m->deps,
                           m->key, r->flags, r->ballot, r->seq, r->deps, m->row);
    else
        hipLaunchKernelGGL(ep_acceptor_kernel<0>, EP_GRID(e), e->v, m->flags, m->peer, m->col, m->ballot, m->seq, m->deps,
                           m->key, r->flags, r->ballot, r->seq, r->deps, m->row);
    SMR_HIP_TRY(hipGetLastError());
    return ep_execute(e, stream);
}

int smr_ep_handle_pre_accept(smr_ep_replica *e, const smr_ep_msg *msg, const smr_ep_msg *reply, void *stream) {
    return ep_acceptor(e, 0, msg, reply, stream);
}

int smr_ep_handle_accept(smr_ep_replica *e, const smr_ep_msg *msg, const smr_ep_msg *reply, void *stream) {
    return ep_acceptor(e, 1, msg, reply, stream);
}

int smr_ep_handle_commit_notice(smr_ep_replica *e, const smr_ep_msg *msg, void *stream) {
    return ep_acceptor(e, 2, msg, nullptr, stream);
}

int smr_ep_handle_pre_accept_replies_at(smr_ep_replica *e, const uint8_t *row_dev, const uint32_t *col_dev,
                                        const uint64_t *ballot_dev, const uint64_t *seq_dev, const uint32_t *deps_dev,
                                        const uint8_t *flags_dev, const uint32_t *order_dev, const uint8_t *exploded_dev,
                                        uint8_t *decision_dev, uint64_t *d_seq_dev, uint32_t *d_deps_dev, void *stream) {
    if (!e || !col_dev || !ballot_dev || !seq_dev || !deps_dev || !flags_dev || !decision_dev || !d_seq_dev || !d_deps_dev)
        return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (row_dev && !e->cfg.recovery) return fail(SMR_ERR_STATE, "epaxos: replies to an instance outside my row need smr_ep_cfg.recovery");
    if (e->v.R <= 5)
        hipLaunchKernelGGL(ep_pre_accept_replies_kernel<5>, EP_GRID(e), e->v, col_dev, ballot_dev, seq_dev, deps_dev, flags_dev,
                           order_dev, exploded_dev, decision_dev, d_seq_dev, d_deps_dev, row_dev);
    else
        hipLaunchKernelGGL(ep_pre_accept_replies_kernel<EMAXR>, EP_GRID(e), e->v, col_dev, ballot_dev, seq_dev, deps_dev,
                           flags_dev, order_dev, exploded_dev, decision_dev, d_seq_dev, d_deps_dev, row_dev);
    SMR_HIP_TRY(hipGetLastError());
    return ep_execute(e, stream);
}

int smr_ep_handle_pre_accept_replies(smr_ep_replica *e, const uint32_t *col_dev, const uint64_t *ballot_dev,
                                     const uint64_t *seq_dev, const uint32_t *deps_dev, const uint8_t *flags_dev,
                                     const uint32_t *order_dev, const uint8_t *exploded_dev, uint8_t *decision_dev,
                                     uint64_t *d_seq_dev, uint32_t *d_deps_dev, void *stream) {
    return smr_ep_handle_pre_accept_replies_at(e, nullptr, col_dev, ballot_dev, seq_dev, deps_dev, flags_dev, order_dev, exploded_dev,
                                               decision_dev, d_seq_dev, d_deps_dev, stream);
}

int smr_ep_leader_handle_wire_pre_accept_replies(smr_ep_replica *e, const uint8_t *buf_dev, uint64_t buf_len, const uint64_t *conn_off_dev,
                                                 const uint8_t *conn_len_dev, uint32_t n_conn, const uint32_t *col_dev, const uint32_t *order_dev,
                                                 const uint8_t *exploded_dev, uint8_t *decision_dev, uint64_t *d_seq_dev, uint32_t *d_deps_dev,
                                                 smr_wire_other *others_dev, uint64_t other_cap, uint64_t *counts_dev, uint64_t *consumed_dev,
                                                 int32_t *status_dev, void *stream) {
    if (!e || !conn_off_dev || !col_dev || !decision_dev || !d_seq_dev || !d_deps_dev || !counts_dev || !consumed_dev || !status_dev ||
        (buf_len && !buf_dev) || (other_cap && !others_dev))
        return fail(SMR_ERR_ARG, "epaxos wire replies: null argument");
    if ((uintptr_t)buf_dev & 15) return fail(SMR_ERR_ARG, "epaxos wire replies: the byte buffer must be 16-byte aligned");
    const uint32_t F = e->v.R - 1u;
    if (n_conn != e->v.G * F)
        return fail(SMR_ERR_ARG, "epaxos wire replies: the connections come dense -- n_groups * (population - 1) of them, connection g * (population - 1) + k "
                                 "= group g's k-th peer in ascending id");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t GPB = EW_BLOCK / F;
    const EpWire A{buf_dev, buf_len, conn_off_dev, conn_len_dev, n_conn, col_dev, order_dev, exploded_dev, decision_dev, d_seq_dev, d_deps_dev,
                   others_dev, other_cap, counts_dev, consumed_dev, status_dev, e->wire_acc};
    const dim3 grid((e->v.G + GPB - 1) / GPB), block(EW_BLOCK);
    if (e->v.R <= 5) hipLaunchKernelGGL(ep_wire_pre_accept_replies_kernel<5>, grid, block, 0, st, e->v, A);
    else hipLaunchKernelGGL(ep_wire_pre_accept_replies_kernel<EMAXR>, grid, block, 0, st, e->v, A);
    int rc = SMR_OK;
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) rc = fail(SMR_ERR_DEVICE, std::string("epaxos wire replies: ") + hipGetErrorString(err));
    else rc = ep_execute(e, stream);
    if (rc != SMR_OK) (void)hipMemsetAsync(e->wire_acc, 0, EW_ACC_WORDS * 8, st);   // (all zero is a state every call can start from)
    return rc;
}

int smr_ep_handle_accept_replies_at(smr_ep_replica *e, const uint8_t *row_dev, const uint32_t *col_dev, const uint64_t *ballot_dev,
                                    const uint8_t *flags_dev, const uint32_t *order_dev, uint8_t *committed_dev, void *stream) {
    if (!e || !col_dev || !ballot_dev || !flags_dev || !committed_dev) return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (row_dev && !e->cfg.recovery) return fail(SMR_ERR_STATE, "epaxos: replies to an instance outside my row need smr_ep_cfg.recovery");
    hipLaunchKernelGGL(ep_accept_replies_kernel, EP_GRID(e), e->v, col_dev, ballot_dev, flags_dev, order_dev, committed_dev, row_dev);
    SMR_HIP_TRY(hipGetLastError());
    return ep_execute(e, stream);
}

int smr_ep_handle_accept_replies(smr_ep_replica *e, const uint32_t *col_dev, const uint64_t *ballot_dev,
                                 const uint8_t *flags_dev, const uint32_t *order_dev, uint8_t *committed_dev, void *stream) {
    return smr_ep_handle_accept_replies_at(e, nullptr, col_dev, ballot_dev, flags_dev, order_dev, committed_dev, stream);
}

int smr_ep_heartbeat_timeout(smr_ep_replica *e, const uint8_t *src_dev, const uint8_t *exploded_dev, uint32_t *n_dev, uint32_t *col_dev,
                             uint64_t *ballot_dev, void *stream) {
    if (!e || !src_dev || !n_dev || !col_dev || !ballot_dev) return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (!e->cfg.recovery) return fail(SMR_ERR_STATE, "epaxos: created without recovery");
    if (e->cfg.execute)
        hipLaunchKernelGGL(ep_heartbeat_timeout_kernel<true>, EP_GRID(e), e->v, e->x, src_dev, exploded_dev, n_dev, col_dev, ballot_dev);
    else
        hipLaunchKernelGGL(ep_heartbeat_timeout_kernel<false>, EP_GRID(e), e->v, e->x, src_dev, exploded_dev, n_dev, col_dev, ballot_dev);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_ep_handle_exp_prepare(smr_ep_replica *e, const smr_ep_exp_prepare *m, const smr_ep_exp_prepare_reply *r, void *stream) {
    if (!e || !m || !r || !m->flags || !m->peer || !m->row || !m->col || !m->new_ballot || !r->flags || !r->voted_bal ||
        !r->voted_status || !r->voted_seq || !r->voted_deps || !r->voted_key)
        return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (!e->cfg.recovery) return fail(SMR_ERR_STATE, "epaxos: created without recovery");
    hipLaunchKernelGGL(ep_exp_prepare_kernel, EP_GRID(e), e->v, m->flags, m->peer, m->row, m->col, m->new_ballot, r->flags,
                       r->voted_bal, r->voted_status, r->voted_seq, r->voted_deps, r->voted_key);
    SMR_HIP_TRY(hipGetLastError());
    return ep_execute(e, stream);                 // (moves no commit bar: the call's submission list becomes empty)
}

int smr_ep_handle_exp_prepare_replies(smr_ep_replica *e, const uint8_t *row_dev, const uint32_t *col_dev, const uint64_t *new_ballot_dev,
                                      const smr_ep_exp_prepare_reply *replies, const uint32_t *order_dev, uint8_t *decision_dev,
                                      uint64_t *d_ballot_dev, uint64_t *d_seq_dev, uint32_t *d_deps_dev, uint8_t *d_key_dev, void *stream) {
    if (!e || !row_dev || !col_dev || !new_ballot_dev || !replies || !replies->flags || !replies->voted_bal || !replies->voted_status ||
        !replies->voted_seq || !replies->voted_deps || !replies->voted_key || !decision_dev || !d_ballot_dev || !d_seq_dev ||
        !d_deps_dev || !d_key_dev)
        return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (!e->cfg.recovery) return fail(SMR_ERR_STATE, "epaxos: created without recovery");
    hipLaunchKernelGGL(ep_exp_prepare_replies_kernel, EP_GRID(e), e->v, row_dev, col_dev, new_ballot_dev, replies->voted_bal,
                       replies->voted_status, replies->voted_seq, replies->voted_deps, replies->voted_key, replies->flags, order_dev,
                       decision_dev, d_ballot_dev, d_seq_dev, d_deps_dev, d_key_dev);
    SMR_HIP_TRY(hipGetLastError());
    return ep_execute(e, stream);
}

int smr_ep_xp_dump(smr_ep_replica *e, uint8_t *acks, uint64_t *max_bal, uint8_t *avoid, uint8_t *has, uint8_t *vstatus, uint64_t *vseq,
                   uint8_t *vkey, uint32_t *vdeps, uint64_t *counters) {
    if (!e || !acks || !max_bal || !avoid || !has || !vstatus || !vseq || !vkey || !vdeps || !counters)
        return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (!e->cfg.recovery) return fail(SMR_ERR_STATE, "epaxos: created without recovery");
    SMR_HIP_TRY(hipDeviceSynchronize());
    const EpView &v = e->v;
    const size_t G = v.G, W = v.W, R = v.R, N = R * W * G;
    std::vector<uint32_t> len(R * G);
    std::vector<uint8_t> a(N), h(N), av(N), bk(N), xs(N * R), xk(N * R);
    std::vector<uint64_t> mx(N), xq(N * R);
    std::vector<uint32_t> xd(N * R * R);
#define D2H(dst, src, n) SMR_HIP_TRY(hipMemcpy((dst), (src), (n), hipMemcpyDeviceToHost))
    D2H(len.data(), v.len, R * G * 4); D2H(mx.data(), v.xp_max, N * 8);
    {                                                                            // the meta words of the instance records (EpView)
        std::vector<uint32_t> p2(N * 4);
        D2H(p2.data(), v.p2, N * 16);
        for (size_t o = 0; o < N; o++) {
            const uint32_t m0 = p2[o * 4 + 1], m1 = p2[o * 4 + 2];
            bk[o] = (uint8_t)(m0 >> 16); av[o] = (uint8_t)(m1 >> 8); a[o] = (uint8_t)(m1 >> 16); h[o] = (uint8_t)(m1 >> 24);
        }
    }
    D2H(xs.data(), v.xv_status, N * R); D2H(xk.data(), v.xv_key, N * R); D2H(xq.data(), v.xv_seq, N * R * 8);
    D2H(xd.data(), v.xv_deps, N * R * R * 4);
#undef D2H
    unsigned long long c[8];
    SMR_HIP_TRY(ctr_read(v.counters, 7, c));
    for (int k = 0; k < 4; k++) counters[k] = c[3 + k];
    // canonical form, like smr_ep_dump: cells outside the last W columns of a row, instances without leader bookkeeping and
    // peers without a voted entry read as empty
    for (size_t row = 0; row < R; row++)
        for (size_t w = 0; w < W; w++)
            for (size_t g = 0; g < G; g++) {
                const size_t o = (row * W + w) * G + g;
                uint32_t cc;
                const bool live = ep_live_col(len[row * G + g], (uint32_t)W, (uint32_t)w, cc);   // (ep_snapshot.h: the live span)
                const bool lb = live && (bk[o] & 1);
                avoid[o] = live ? av[o] : 0; acks[o] = lb ? a[o] : 0; max_bal[o] = lb ? mx[o] : 0; has[o] = lb ? h[o] : 0;
                for (size_t p = 0; p < R; p++) {
                    const size_t q = ((row * W + w) * R + p) * G + g;
                    const bool on = lb && ((h[o] >> p) & 1);
                    vstatus[q] = on ? xs[q] : 0; vseq[q] = on ? xq[q] : 0; vkey[q] = on ? xk[q] : 0xFF;
                    for (size_t i = 0; i < R; i++) {
                        const size_t z = (((row * W + w) * R + p) * R + i) * G + g;
                        vdeps[z] = on ? xd[z] : 0xFFFFFFFFu;
                    }
                }
            }
    return SMR_OK;
}

int smr_ep_dump(smr_ep_replica *e, const smr_ep_dump_bufs *hb) {
    if (!e || !hb) return fail(SMR_ERR_ARG, "epaxos: null argument");
    SMR_HIP_TRY(hipDeviceSynchronize());
    const EpView &v = e->v;
    const size_t G = v.G, W = v.W, R = v.R, K = v.n_keys;
#define D2H(dst, src, n) SMR_HIP_TRY(hipMemcpy((dst), (src), (n), hipMemcpyDeviceToHost))
    D2H(hb->len, v.len, R * G * 4); D2H(hb->commit_bars, v.commit_bars, R * G * 4);
    {                                                                            // device [G][K][R] -> the dump's [K][R][G]
        const size_t EW = v.hc_es;                                               // (a cluster's shared table: this replica's slot of every entry, the
        std::vector<uint32_t> hc(K * EW * G);                                    // view's base pointing at it)
        D2H(hc.data(), v.hc, (K * EW * G - (EW - v.hc_ew)) * 4);
        for (size_t g = 0; g < G; g++)
            for (size_t k = 0; k < K; k++)
                for (size_t r = 0; r < R; r++) hb->highest_cols[(k * R + r) * G + g] = hc[(g * K + k) * EW + r];
    }
    std::vector<uint64_t> bal(R * W * G), seq(R * W * G);
    std::vector<uint8_t> st(R * W * G), key(R * W * G), bk(R * W * G), pa(R * W * G), ac(R * W * G);
    std::vector<uint32_t> deps(R * W * R * G);
    {                                                                            // the instance records (EpView), unpacked to the planes of the dump
        const size_t N = R * W * G;
        std::vector<uint32_t> p0(N * 4), p1(N * 4), p2(N * 4), p3(R > 6 ? N * 4 : 0);
        D2H(p0.data(), v.p0, N * 16); D2H(p1.data(), v.p1, N * 16); D2H(p2.data(), v.p2, N * 16);
        if (R > 6) D2H(p3.data(), v.p3, N * 16);
        for (size_t rw = 0; rw < R * W; rw++)
            for (size_t g = 0; g < G; g++) {
                const size_t o = rw * G + g;
                bal[o] = (uint64_t)p0[o * 4] | ((uint64_t)p0[o * 4 + 1] << 32);
                seq[o] = (uint64_t)p0[o * 4 + 2] | ((uint64_t)p0[o * 4 + 3] << 32);
                const uint32_t m0 = p2[o * 4 + 1], m1 = p2[o * 4 + 2];
                st[o] = (uint8_t)m0; key[o] = (uint8_t)(m0 >> 8); bk[o] = (uint8_t)(m0 >> 16); pa[o] = (uint8_t)(m0 >> 24); ac[o] = (uint8_t)m1;
                for (size_t i = 0; i < R; i++) {
                    const uint32_t d = i < 4 ? p1[o * 4 + i] : i == 4 ? p2[o * 4] : i == 5 ? p2[o * 4 + 3] : p3[o * 4 + (i - 6)];
                    deps[(rw * R + i) * G + g] = d;
                }
            }
    }
    unsigned long long c[4];
    SMR_HIP_TRY(ctr_read(v.counters, 4, c));   // (explicit-prepare outcomes: smr_ep_xp_dump)
#undef D2H
    hb->counters[0] = c[0]; hb->counters[1] = c[1]; hb->counters[2] = c[2];
    // canonical form: only the last W columns of each row are state; deps as [row][w][g][i]
    for (size_t row = 0; row < R; row++)
        for (size_t w = 0; w < W; w++)
            for (size_t g = 0; g < G; g++) {
                const size_t o = (row * W + w) * G + g;
                uint32_t cc;                                                     // the column this cell holds, if any
                const bool live = ep_live_col(hb->len[row * G + g], (uint32_t)W, (uint32_t)w, cc);   // (ep_snapshot.h: the live span)
                hb->bal[o] = live ? bal[o] : 0; hb->seq[o] = live ? seq[o] : 0; hb->status[o] = live ? st[o] : 0;
                hb->key[o] = live ? key[o] : 0xFF; hb->pa_acks[o] = live ? pa[o] : 0; hb->acc_acks[o] = live ? ac[o] : 0;
                hb->bk[o] = live ? bk[o] : 0;
                for (size_t i = 0; i < R; i++) hb->deps[o * R + i] = live ? deps[((row * W + w) * R + i) * G + g] : 0xFFFFFFFFu;
            }
    return SMR_OK;
}

int smr_ep_exec_dump(smr_ep_replica *e, uint32_t *exec_bars, uint64_t *kv, uint64_t *digest, uint64_t *counters) {
    if (!e || !exec_bars || !kv || !digest || !counters) return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (!e->cfg.execute) return fail(SMR_ERR_ARG, "epaxos: created without execution");
    SMR_HIP_TRY(hipDeviceSynchronize());
    const EpView &v = e->v;
    const size_t G = v.G, R = v.R, K = v.n_keys;
    SMR_HIP_TRY(hipMemcpy(exec_bars, e->x.exec_bars, R * G * 4, hipMemcpyDeviceToHost));
    {                                                                            // device: in the hc entries [G][K][hc_es] -> the dump's [K][G]
        const size_t EW = v.hc_es;
        std::vector<uint32_t> hc(K * EW * G);
        SMR_HIP_TRY(hipMemcpy(hc.data(), v.hc, (K * EW * G - (EW - v.hc_ew)) * 4, hipMemcpyDeviceToHost));
        for (size_t g = 0; g < G; g++)
            for (size_t k = 0; k < K; k++) kv[k * G + g] = ep_kv_unpack(hc[(g * K + k) * EW + v.hc_kv]);
    }
    SMR_HIP_TRY(hipMemcpy(digest, e->x.digest, G * 8, hipMemcpyDeviceToHost));
    unsigned long long c[8];
    SMR_HIP_TRY(ctr_read(e->x.counters, 8, c));
    for (int k = 0; k < 6; k++) counters[k] = c[k];
    counters[3] = 0;                                                             // (the dump's slot 3 stays the reference's unused counter)
    if (c[3]) return fail(SMR_ERR_STATE, "epaxos: " + std::to_string(c[3]) + " instances were executed at a column >= 2^28: the 32-bit KV words of the per-key "
                                         "table cannot hold their tokens (start a fresh replica object; ep_kv_pack)");
    return SMR_OK;
}

int smr_ep_exec_poll(smr_ep_replica *e, uint32_t *group_host, uint8_t *row_host, uint32_t *col_host, uint64_t cap, uint64_t *n_out) {
    if (!e || !n_out) return fail(SMR_ERR_ARG, "epaxos: null argument");
    if (!e->cfg.execute) return fail(SMR_ERR_ARG, "epaxos: created without execution");
    SMR_HIP_TRY(hipDeviceSynchronize());
    const EpView &v = e->v;
    const size_t G = v.G, R = v.R;
    std::vector<uint32_t> n_sub(G), len(R * G);
    SMR_HIP_TRY(hipMemcpy(n_sub.data(), e->x.n_sub, G * 4, hipMemcpyDeviceToHost));
    SMR_HIP_TRY(hipMemcpy(len.data(), v.len, R * G * 4, hipMemcpyDeviceToHost));
    uint32_t most = 0;
    for (size_t g = 0; g < G; g++) most = n_sub[g] > most ? n_sub[g] : most;
    std::vector<uint16_t> order((size_t)most * G);
    if (most) SMR_HIP_TRY(hipMemcpy(order.data(), e->x.order, (size_t)most * G * 2, hipMemcpyDeviceToHost));
    uint32_t wshift = 0;
    while ((1u << wshift) < v.W) wshift++;
    uint64_t n = 0;
    for (size_t g = 0; g < G; g++)
        for (uint32_t k = 0; k < n_sub[g]; k++, n++) {
            if (n >= cap || !group_host || !row_host || !col_host) continue;
            const uint32_t ring = order[(size_t)k * G + g], row = ring >> wshift, w = ring & v.Wmask;
            uint32_t col;                                                    // the column of that residue among the last W
            (void)ep_live_col(len[row * G + g], v.W, w, col);
            group_host[n] = (uint32_t)g; row_host[n] = (uint8_t)row; col_host[n] = col;
        }
    *n_out = n;
    if (group_host && row_host && col_host) SMR_HIP_TRY(hipMemset(e->x.n_sub, 0, G * 4));   // a count-only call leaves them
    {
        unsigned long long c[8];
        SMR_HIP_TRY(ctr_read(e->x.counters, 8, c));
        if (c[3]) return fail(SMR_ERR_STATE, "epaxos: an instance was executed at a column >= 2^28: its token does not fit the 32-bit KV word (ep_kv_pack)");
    }
    return SMR_OK;
}

#ifdef EPC_STAMPS
static unsigned long long *g_epc_stamps = nullptr;
static size_t g_epc_stamps_n = 0;
int smr_dbg_epc_stamps(unsigned long long *host, size_t cap) {      // experiments only: the last tick's per-step wall-clock stamps (100 MHz)
    if (!g_epc_stamps || cap < g_epc_stamps_n) return SMR_ERR_ARG;
    SMR_HIP_TRY(hipDeviceSynchronize());
    SMR_HIP_TRY(hipMemcpy(host, g_epc_stamps, g_epc_stamps_n * 8, hipMemcpyDeviceToHost));
    return (int)g_epc_stamps_n;
}
#endif
/* ---- one tick of a co-located EPaxos cluster as ONE call: one launch (ep_cluster_tick_kernel), or -- mode 1 -- the handler
 * kernels back to back, launch by launch, as summerset_amd/ep_cluster.py's closed loop drives them ---- */
struct smr_ep_cluster {
    uint32_t R = 0, G = 0, mode = 0;
    smr_ep_replica *rep[SMR_MAX_REPLICAS] = {};
    char *base = nullptr;
    // per command leader s (all device): the PreAcceptReplies / AcceptReplies of its peers stacked by peer id ([s][q][G]: the
    // one-launch tick indexes them from r_flags[0] / r_seq[0] / r_deps[0] / a_flags[0]), its flag arrays (mode 1)
    uint8_t *r_flags[SMR_MAX_REPLICAS], *a_flags[SMR_MAX_REPLICAS], *slow[SMR_MAX_REPLICAS], *acc[SMR_MAX_REPLICAS], *peer_c[SMR_MAX_REPLICAS];
    uint8_t *masked;                                         // the PreAccept's flags behind a drop mask
    uint64_t *r_ballot[SMR_MAX_REPLICAS], *r_seq[SMR_MAX_REPLICAS], *a_ballot[SMR_MAX_REPLICAS], *bal_c[SMR_MAX_REPLICAS];
    uint32_t *r_deps[SMR_MAX_REPLICAS];
    // the shared per-key table (see ep_hc_migrate_kernel; NULL: the replicas keep their private tables -- populations > 5, or a
    // table that would pass the 32-bit offsets) and what the replicas' views held before
    uint32_t *hc_shared = nullptr;
    uint32_t *hc_priv[SMR_MAX_REPLICAS] = {};
    uint32_t hc_priv_ew = 0, hc_priv_kv = 0;
    uint32_t *defer_cnt = nullptr, *defer_list = nullptr;    // ep_cluster_tick_pm_kernel's lists (EpClusterArgs)
    uint32_t parity = 0;
    bool unbatched = false;                                  // SMR_EP_PM_UNBATCHED (A/B runs): the phase-by-phase order on the step-by-step kernel
};
constexpr uint32_t EP_HC_SHARED_ES = 32;                 // words between two keys' entries of the shared table: one 128-byte line

int smr_ep_cluster_create(smr_ep_replica *const *reps, uint32_t n, smr_ep_cluster **out) {
    if (!reps || !out) return fail(SMR_ERR_ARG, "epaxos cluster: null argument");
    if (n < 3 || n > SMR_MAX_REPLICAS) return fail(SMR_ERR_ARG, "epaxos cluster: 3..8 replicas");
    for (uint32_t r = 0; r < n; r++) {
        if (!reps[r]) return fail(SMR_ERR_ARG, "epaxos cluster: null replica");
        const smr_ep_cfg &k = reps[r]->cfg, &k0 = reps[0]->cfg;
        if (k.population != n || k.me != r || k.n_groups != k0.n_groups)
            return fail(SMR_ERR_ARG, "epaxos cluster: replica r must be created with me = r, population = n and the same groups");
        // the tick's message layout and its execution-pass rule are the cluster's, not a replica's: a mixed cluster would
        // quietly leave the handler-by-handler loop
        if (k.window != k0.window || k.n_keys != k0.n_keys || k.execute != k0.execute || k.recovery != k0.recovery ||
            k.optimized_quorum != k0.optimized_quorum)
            return fail(SMR_ERR_ARG, "epaxos cluster: the replicas must agree in window, n_keys, execute, recovery and optimized_quorum");
    }
    smr_ep_cluster *c = new smr_ep_cluster();
    c->R = n; c->G = reps[0]->cfg.n_groups;
    c->unbatched = getenv("SMR_EP_PM_UNBATCHED") != nullptr;
    for (uint32_t r = 0; r < n; r++) c->rep[r] = reps[r];
    const size_t G = c->G, R = n;
    // 8-byte arrays first; everything zero: a leader's own row of the stacks is never written and never read as a reply.
    // Each kind of stack is ONE array over the leaders ([s][q]...), the per-leader pointers are views of it.
    const size_t n64 = R * (R * G) * 3 + R * G, n32 = R * (R * R * G) + R * G + 2 * SMR_MAX_REPLICAS * 32, n8 = R * (R * G) * 2 + R * G * 3 + G;
    const size_t bytes = n64 * 8 + n32 * 4 + n8 + 4096;
    if (hipMalloc((void **)&c->base, bytes) != hipSuccess) { delete c; return fail(SMR_ERR_DEVICE, "epaxos cluster: hipMalloc failed"); }
    if (hipMemset(c->base, 0, bytes) != hipSuccess) { (void)hipFree(c->base); delete c; return fail(SMR_ERR_DEVICE, "epaxos cluster: hipMemset failed"); }
    uint64_t *p64 = (uint64_t *)c->base;
    for (uint32_t s = 0; s < R; s++) { c->r_ballot[s] = p64; p64 += R * G; }
    for (uint32_t s = 0; s < R; s++) { c->r_seq[s] = p64; p64 += R * G; }
    for (uint32_t s = 0; s < R; s++) { c->a_ballot[s] = p64; p64 += R * G; }
    for (uint32_t s = 0; s < R; s++) { c->bal_c[s] = p64; p64 += G; }
    uint32_t *p32 = (uint32_t *)p64;
    for (uint32_t s = 0; s < R; s++) { c->r_deps[s] = p32; p32 += R * R * G; }
    c->defer_list = p32; p32 += R * G;
    c->defer_cnt = p32; p32 += 2 * SMR_MAX_REPLICAS * 32;
    uint8_t *p8 = (uint8_t *)p32;
    for (uint32_t s = 0; s < R; s++) { c->r_flags[s] = p8; p8 += R * G; }
    for (uint32_t s = 0; s < R; s++) { c->a_flags[s] = p8; p8 += R * G; }
    for (uint32_t s = 0; s < R; s++) { c->slow[s] = p8; p8 += G; c->acc[s] = p8; p8 += G; c->peer_c[s] = p8; p8 += G; }
    c->masked = p8;
    void *stream = nullptr;
    for (uint32_t s = 0; s < R; s++)
        hipLaunchKernelGGL(ep_fill_kernel, dim3((c->G + 255) / 256), dim3(256), 0, (hipStream_t)stream, c->G, c->peer_c[s], (uint8_t)s, c->bal_c[s],
                           (uint64_t)(s + 1));
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(c->base); delete c;
        return fail(SMR_ERR_DEVICE, "epaxos cluster: initialisation failed");
    }
    // one per-key table for the whole cluster, where R slots of R + 1 words fit a line and the table the 32-bit offsets; a replica
    // that already sits in another cluster's table (its entry stride says so) keeps what it has
    const uint64_t K = reps[0]->cfg.n_keys, tbytes = (uint64_t)G * K * EP_HC_SHARED_ES * 4;
    bool share = R * (R + 1) <= EP_HC_SHARED_ES && tbytes < (1ull << 32) && getenv("SMR_EP_PRIVATE_HC") == nullptr;
    for (uint32_t r = 0; r < R; r++) share = share && reps[r]->v.hc_es == reps[r]->v.hc_ew;
    if (share && hipMalloc((void **)&c->hc_shared, tbytes) == hipSuccess) {
        bool ok = hipMemset(c->hc_shared, 0xFF, tbytes) == hipSuccess;
        c->hc_priv_ew = reps[0]->v.hc_ew; c->hc_priv_kv = reps[0]->v.hc_kv;
        const uint32_t n_entries = (uint32_t)(G * K);
        for (uint32_t r = 0; r < R && ok; r++) {
            EpView &v = reps[r]->v;
            c->hc_priv[r] = v.hc;
            uint32_t *slot0 = c->hc_shared + (size_t)r * (R + 1);
            hipLaunchKernelGGL(ep_hc_migrate_kernel, dim3((n_entries + 255) / 256), dim3(256), 0, (hipStream_t)stream, v.hc, v.hc_es, v.hc_kv, slot0,
                               EP_HC_SHARED_ES, (uint32_t)R, n_entries, 1);
            ok = hipGetLastError() == hipSuccess;
        }
        ok = ok && hipDeviceSynchronize() == hipSuccess;
        if (!ok) {
            (void)hipFree(c->hc_shared); (void)hipFree(c->base); delete c;
            return fail(SMR_ERR_DEVICE, "epaxos cluster: the shared per-key table could not be filled");
        }
        for (uint32_t r = 0; r < R; r++) {                       // from here on every kernel of replica r -- its own handlers too -- works in its slot
            EpView &v = reps[r]->v;
            reps[r]->seat = &c->rep[r];
            v.hc = c->hc_shared + (size_t)r * (R + 1);
            v.hc_es = EP_HC_SHARED_ES; v.hc_ew = (uint32_t)R + 1u; v.hc_kv = (uint32_t)R;
        }
    } else {
        c->hc_shared = nullptr;
    }
    *out = c;
    return SMR_OK;
}

void smr_ep_cluster_destroy(smr_ep_cluster *c) {
    if (!c) return;
    if (c->hc_shared) {                                          // the replicas outlive the cluster: their entries go back into their own tables
        (void)hipDeviceSynchronize();
        const uint32_t n_entries = c->G * c->rep[0]->cfg.n_keys;
        for (uint32_t r = 0; r < c->R; r++) {
            if (!c->rep[r]) continue;                            // that replica is gone already
            c->rep[r]->seat = nullptr;
            EpView &v = c->rep[r]->v;
            hipLaunchKernelGGL(ep_hc_migrate_kernel, dim3((n_entries + 255) / 256), dim3(256), 0, (hipStream_t)nullptr, c->hc_priv[r], c->hc_priv_ew,
                               c->hc_priv_kv, v.hc, EP_HC_SHARED_ES, c->R, n_entries, 0);
            v.hc = c->hc_priv[r]; v.hc_es = v.hc_ew = c->hc_priv_ew; v.hc_kv = c->hc_priv_kv;
        }
        (void)hipDeviceSynchronize();
        (void)hipFree(c->hc_shared);
    }
    if (c->base) (void)hipFree(c->base);
    delete c;
}

int smr_ep_cluster_batch_stats(smr_ep_cluster *c, uint64_t out[2]) {
    if (!c || !out) return fail(SMR_ERR_ARG, "epaxos cluster: null argument");
    out[0] = out[1] = 0;
    for (uint32_t r = 0; r < c->R; r++) {
        if (!c->rep[r]) return fail(SMR_ERR_STATE, "epaxos cluster: a replica of this cluster was destroyed");
        unsigned long long k[8];
        SMR_HIP_TRY(hipDeviceSynchronize());
        SMR_HIP_TRY(ctr_read(c->rep[r]->v.counters, 8, k));
        out[0] += k[7] & 0xFFFFFFFFull; out[1] += k[7] >> 32;
    }
    return SMR_OK;
}

int smr_ep_cluster_set_mode(smr_ep_cluster *c, uint32_t mode) {
    if (!c) return fail(SMR_ERR_ARG, "epaxos cluster: null argument");
    if (mode > 3) return fail(SMR_ERR_ARG, "epaxos cluster: mode must be 0 .. 3 (bit 0: one launch per handler, bit 1: the leaders' steps phase by phase)");
    c->mode = mode;
    return SMR_OK;
}

}  // extern "C"

template <int NR>
static int ep_cluster_tick_one_launch(smr_ep_cluster *c, const uint8_t *const *keys_dev, const uint8_t *const *drop_dev,
                                      const smr_ep_cluster_out *out, void *stream) {
    const uint32_t R = c->R, G = c->G;
    EpClusterArgs<NR> a;
    memset(&a, 0, sizeof(a));
    a.R = R; a.G = G; a.execute = c->rep[0]->cfg.execute; a.quiet = !c->rep[0]->cfg.recovery;
    a.phase_major = (c->mode >> 1) & 1u;
    a.v0 = c->rep[0]->v; a.x0 = c->rep[0]->x;
    // (read off the views, not off c->hc_shared: the table may be another cluster's of the same replicas)
    a.hc_slot_bytes = c->rep[0]->v.hc_es != c->rep[0]->v.hc_ew ? (R + 1u) * 4u : 0u;
    for (uint32_t r = 0; r < R; r++) {
        if (a.hc_slot_bytes ? c->rep[r]->v.hc != c->rep[0]->v.hc + (size_t)r * (R + 1u) || c->rep[r]->v.hc_es != c->rep[0]->v.hc_es
                            : c->rep[r]->v.hc_es != c->rep[r]->v.hc_ew)
            return fail(SMR_ERR_STATE, "epaxos cluster: the replicas' per-key tables are not one cluster's");
        a.delta[r] = (int64_t)(c->rep[r]->arena.base - c->rep[0]->arena.base);
        // (one layout: smr_ep_cluster_create took only replicas that agree in everything the layout depends on)
        if ((char *)c->rep[r]->v.p0 - c->rep[r]->arena.base != (char *)c->rep[0]->v.p0 - c->rep[0]->arena.base ||
            (char *)c->rep[r]->v.counters - c->rep[r]->arena.base != (char *)c->rep[0]->v.counters - c->rep[0]->arena.base)
            return fail(SMR_ERR_STATE, "epaxos cluster: the replicas' arenas differ in layout");
        a.keys[r] = keys_dev[r]; a.out[r] = out[r];
        for (uint32_t q = 0; q < R; q++) a.drop[r * NR + q] = drop_dev ? drop_dev[(size_t)r * R + q] : nullptr;
    }
    a.r_flags = c->r_flags[0]; a.a_flags = c->a_flags[0]; a.r_seq = c->r_seq[0]; a.r_deps = c->r_deps[0];
#ifdef EPC_STAMPS
    static unsigned long long *g_stamps = nullptr;
    if (!g_stamps) { SMR_HIP_TRY(hipMalloc((void **)&g_stamps, 8 * NR * 64 * 8)); }
    SMR_HIP_TRY(hipMemsetAsync(g_stamps, 0, 8 * NR * 64 * 8, (hipStream_t)stream));
    a.stamps = g_stamps;
    g_epc_stamps = g_stamps; g_epc_stamps_n = 8 * NR * 64;
#endif
    if (a.quiet && a.phase_major && NR <= 5 && !c->unbatched) {
        // (NR > 5 never gets here; the instantiation is kept out of the 8-replica build by the constant)
        if constexpr (NR <= 5) {
            a.defer_cnt = c->defer_cnt; a.defer_list = c->defer_list; a.parity = c->parity;
            c->parity ^= 1u;
            hipLaunchKernelGGL((ep_cluster_tick_pm_kernel<NR>), dim3((G + 64 * epc_sets<NR>() - 1) / (64 * epc_sets<NR>())), dim3(R * 64 * epc_sets<NR>()), 0,
                               (hipStream_t)stream, a);
            hipLaunchKernelGGL((ep_cluster_commit_one_by_one_kernel<NR>), dim3(R, std::min<uint32_t>((G + EPC_CL_LANES - 1u) / EPC_CL_LANES, EPC_CL_MAX_BLOCKS)), dim3(64), 0, (hipStream_t)stream, a);
        }
    } else if (a.quiet)
        hipLaunchKernelGGL((ep_cluster_tick_kernel<NR, false>), dim3((G + 64 * epc_sets<NR>() - 1) / (64 * epc_sets<NR>())), dim3(R * 64 * epc_sets<NR>()), 0,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((ep_cluster_tick_kernel<NR, true>), dim3((G + 64 * epc_sets<NR>() - 1) / (64 * epc_sets<NR>())), dim3(R * 64 * epc_sets<NR>()), 0,
                           (hipStream_t)stream, a);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

extern "C" {

int smr_ep_cluster_tick(smr_ep_cluster *c, const uint8_t *const *keys_dev, const uint8_t *const *drop_dev, const smr_ep_cluster_out *out,
                        void *stream) {
    if (!c || !keys_dev || !out) return fail(SMR_ERR_ARG, "epaxos cluster: null argument");
    const uint32_t R = c->R, G = c->G;
    for (uint32_t s = 0; s < R; s++)
        if (!c->rep[s]) return fail(SMR_ERR_STATE, "epaxos cluster: a replica of this cluster was destroyed");
    for (uint32_t s = 0; s < R; s++)
        if (!keys_dev[s] || !out[s].proposed || !out[s].col || !out[s].seq0 || !out[s].deps0 || !out[s].decision || !out[s].committed ||
            !out[s].seq || !out[s].deps)
            return fail(SMR_ERR_ARG, "epaxos cluster: null key or output array");
    if ((c->mode & 1u) == 0)
        return R <= 5 ? ep_cluster_tick_one_launch<5>(c, keys_dev, drop_dev, out, stream)
                      : ep_cluster_tick_one_launch<EMAXR>(c, keys_dev, drop_dev, out, stream);
    const dim3 grid((G + 255) / 256), block(256);
    int rc;
    // mode 1, launch by launch.  With execution on every handler is followed by the execution kernel, which does something only where a commit bar
    // moved.  A proposal (the leader's own reply alone is below any quorum) and an acceptor's PreAccept / Accept handling
    // (no commit; its leader-bookkeeping branch exists only under explicit prepare) move none, so the 45 launches behind
    // them are left out -- unless the replica was created with recovery.  (smr_ep_exec_poll then reports the tick's last
    // handler, a CommitNotice, as before.)
    struct NoExec {
        smr_ep_replica *e;
        explicit NoExec(smr_ep_replica *e_) : e(e_) { e->skip_exec = !e->cfg.recovery; }
        ~NoExec() { e->skip_exec = false; }
    };
    // every replica proposes; the PreAccept it broadcasts lies in the caller's arrays
    for (uint32_t s = 0; s < R; s++) {
        smr_ep_msg pa{out[s].proposed, nullptr, out[s].col, nullptr, out[s].seq0, out[s].deps0, nullptr, nullptr};
        NoExec ne(c->rep[s]);
        if ((rc = smr_ep_propose(c->rep[s], keys_dev[s], nullptr, &pa, stream)) != SMR_OK) return rc;
    }
    // acceptors: one sender's PreAccept at a time, senders ascending; the reply goes straight into row q of the sender's stack
    for (uint32_t q = 0; q < R; q++)
        for (uint32_t s = 0; s < R; s++) {
            if (s == q) continue;
            uint8_t *fl = out[s].proposed;
            const uint8_t *dm = drop_dev ? drop_dev[(size_t)s * R + q] : nullptr;
            if (dm) {
                hipLaunchKernelGGL(ep_flags_drop_kernel, grid, block, 0, (hipStream_t)stream, G, out[s].proposed, dm, c->masked);
                fl = c->masked;
            }
            smr_ep_msg m{fl, c->peer_c[s], out[s].col, c->bal_c[s], out[s].seq0, out[s].deps0, (uint8_t *)keys_dev[s], nullptr};
            smr_ep_msg r{c->r_flags[s] + (size_t)q * G, nullptr, nullptr, c->r_ballot[s] + (size_t)q * G, c->r_seq[s] + (size_t)q * G,
                         c->r_deps[s] + (size_t)q * R * G, nullptr, nullptr};
            NoExec ne(c->rep[q]);
            if ((rc = smr_ep_handle_pre_accept(c->rep[q], &m, &r, stream)) != SMR_OK) return rc;
        }
    // command leaders, ascending: decision; the Accept round (flags zero where the fast path was taken); CommitNotices -- leader by
    // leader, or (mode bit 1) phase by phase: every leader's decision, then every Accept round, ...
    const bool pm = (c->mode >> 1) & 1u;
    for (uint32_t ph = 0; ph < (pm ? 4u : 1u); ph++)
        for (uint32_t s = 0; s < R; s++) {
            if (!pm || ph == 0) {
                if ((rc = smr_ep_handle_pre_accept_replies(c->rep[s], out[s].col, c->r_ballot[s], c->r_seq[s], c->r_deps[s], c->r_flags[s], nullptr,
                                                           nullptr, out[s].decision, out[s].seq, out[s].deps, stream)) != SMR_OK) return rc;
                hipLaunchKernelGGL(ep_flags_eq_kernel, grid, block, 0, (hipStream_t)stream, G, out[s].decision, (uint8_t)2, (const uint8_t *)nullptr,
                                   (uint8_t)0, c->slow[s]);
            }
            if (!pm || ph == 1)
                for (uint32_t q = 0; q < R; q++) {
                    if (q == s) continue;
                    smr_ep_msg m{c->slow[s], c->peer_c[s], out[s].col, c->bal_c[s], out[s].seq, out[s].deps, (uint8_t *)keys_dev[s], nullptr};
                    smr_ep_msg r{c->a_flags[s] + (size_t)q * G, nullptr, nullptr, c->a_ballot[s] + (size_t)q * G, nullptr, nullptr, nullptr, nullptr};
                    NoExec ne(c->rep[q]);
                    if ((rc = smr_ep_handle_accept(c->rep[q], &m, &r, stream)) != SMR_OK) return rc;
                }
            if (!pm || ph == 2) {
                if ((rc = smr_ep_handle_accept_replies(c->rep[s], out[s].col, c->a_ballot[s], c->a_flags[s], nullptr, c->acc[s], stream)) != SMR_OK) return rc;
                hipLaunchKernelGGL(ep_flags_eq_kernel, grid, block, 0, (hipStream_t)stream, G, out[s].decision, (uint8_t)3, c->acc[s], (uint8_t)1,
                                   out[s].committed);
            }
            if (!pm || ph == 3)
                for (uint32_t q = 0; q < R; q++) {
                    if (q == s) continue;
                    smr_ep_msg m{out[s].committed, c->peer_c[s], out[s].col, c->bal_c[s], out[s].seq, out[s].deps, (uint8_t *)keys_dev[s], nullptr};
                    if ((rc = smr_ep_handle_commit_notice(c->rep[q], &m, stream)) != SMR_OK) return rc;
                }
        }
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}


}  // extern "C"

/* ---- save / load of one replica's state on the device (ep_snapshot.h: the image and its two kernels) ----------------------------
 * A batched replica object is saved and brought back whole, between two handler calls, by one kernel each, while the other
 * replicas of its cluster go on: a checkpoint, the restart of one replica, the way back from an aborted L2 tick. */
struct smr_ep_snapshot : SnapObj<EpSnapHdr, 3> {                 // cap: cells, reply records, submission-list entries
    uint32_t G = 0, K = 0;
    uint8_t R = 0, me = 0, oq = 0, execute = 0, recovery = 0;
};

namespace smr {
static EpSnapGeom epsnap_geom_of(const smr_ep_snapshot *s) { return epsnap_geom(s->G, s->R, s->K, s->execute, s->recovery); }
static EpSnapImg epsnap_img(const smr_ep_snapshot *s) { return EpSnapImg{s->buf.dev, s->cap[0], s->cap[1], s->cap[2]}; }
// made for a replica of c's kind, whatever its n_groups (a snapshot of chosen groups has its own)
static bool epsnap_like_kind(const smr_ep_snapshot *s, const smr_ep_cfg &c) {
    return s->R == c.population && s->me == c.me && s->oq == (c.optimized_quorum ? 1 : 0) && s->execute == c.execute && s->recovery == c.recovery &&
           s->K == c.n_keys;
}
static bool epsnap_like(const smr_ep_snapshot *s, const smr_ep_cfg &c) { return s->G == c.n_groups && epsnap_like_kind(s, c); }
static bool epsnap_hdr_like_kind(const EpSnapHdr &h, const smr_ep_snapshot *s) {
    return h.population == s->R && h.me == s->me && h.optimized_quorum == s->oq && h.execute == s->execute && h.recovery == s->recovery && h.n_keys == s->K;
}
static bool epsnap_hdr_like(const EpSnapHdr &h, const smr_ep_snapshot *s) { return h.n_groups == s->G && epsnap_hdr_like_kind(h, s); }
static const char *const EPSNAP_OTHER = "another n_groups / population / replica id / optimized_quorum / execute / recovery / n_keys";
static const char *const EPSNAP_OTHER_KIND = "another population / replica id / optimized_quorum / execute / recovery / n_keys";   // (the listed-groups calls)

// what is EPaxos's own of a snapshot object and its calls (snapshot_common.h: SnapObj)
struct EpSnap {
    static constexpr const char *WHAT = "epaxos snapshot: ", *GWHAT = "epaxos groups: ", *NOUN = "replica", *LIST_OF = "";
    static constexpr bool LIST_FIRST = false;
    static uint32_t groups_of(const smr_ep_replica *e) { return e->cfg.n_groups; }
    static int init(smr_ep_snapshot *s, const smr_ep_replica *like) {
        const smr_ep_cfg &c = like->cfg;
        s->K = c.n_keys; s->R = c.population; s->me = c.me; s->oq = c.optimized_quorum ? 1 : 0; s->execute = c.execute; s->recovery = c.recovery;
        return SMR_OK;
    }
    // every ring cell live, the submission list full
    static void need(const smr_ep_snapshot *s, const smr_ep_replica *e, uint64_t (&n)[3]) {
        const uint64_t W = e->cfg.window;
        n[0] = (uint64_t)s->G * s->R * W; n[1] = (uint64_t)s->G * (s->recovery ? s->R : 1) * W; n[2] = s->execute ? 2 * n[0] : 0;
    }
    static void counts(const EpSnapHdr &h, uint64_t (&n)[3]) { n[0] = h.n_cells; n[1] = h.n_replies; n[2] = h.n_exec; }
    static uint64_t dev_bytes(const smr_ep_snapshot *s) { return epsnap_dev_bytes(epsnap_geom_of(s), epsnap_img(s)); }
    static int copy(const smr_ep_snapshot *s, uint8_t *host, const EpSnapHdr &h, bool to_host) {
        const EpSnapGeom q = epsnap_geom_of(s);
        const uint64_t bc = h.n_cells * sizeof(EpSnapCell), br = (uint64_t)h.n_replies * q.r_stride, bx = h.n_exec * sizeof(EpSnapExec);
        return snap_copy_sections(s->buf.dev, host, q.fixed, to_host,
                                  {{q.fixed, bc, bc}, {epsnap_off_rep(q, epsnap_img(s)), br, br}, {epsnap_off_exec(q, epsnap_img(s)), bx, bx}});
    }
    // groups: the image's n_groups is the snapshot's and the list's length (groups_pair_check), the replica's own is free
    static int load_fits(const smr_ep_snapshot *s, const smr_ep_replica *e, const char *what, bool groups) {
        if (groups) {
            if (!epsnap_hdr_like_kind(s->hdr, s)) return fail(SMR_ERR_ARG, std::string(what) + "the image is of " + EPSNAP_OTHER_KIND);
            if (int rc = snap_groups_len_check(s->hdr.n_groups, s->G, what)) return rc;
        } else if (!epsnap_hdr_like(s->hdr, s)) return fail(SMR_ERR_ARG, std::string(what) + "the image is of " + EPSNAP_OTHER);
        // a cell is held iff column + W >= len: in another ring the cells around the saved span would count as held or lost
        if (s->hdr.window != e->cfg.window)
            return fail(SMR_ERR_ARG, std::string(what) + "an image of window " + std::to_string(s->hdr.window) + " does not load into window " + std::to_string(e->cfg.window));
        return SMR_OK;
    }
    static int replica_check(smr_ep_replica *const *reps, uint32_t k, const char *what) {
        const smr_ep_cfg &c = reps[k]->cfg, &c0 = reps[0]->cfg;
        if (c.n_groups != c0.n_groups || c.population != c0.population || c.n_keys != c0.n_keys || c.execute != c0.execute || c.recovery != c0.recovery)
            return fail(SMR_ERR_ARG, std::string(what) + "the replicas differ in groups / population / n_keys / execute / recovery");
        return SMR_OK;
    }
    static int pair_check(smr_ep_replica *const *reps, smr_ep_snapshot *const *snaps, uint32_t k) {
        if (int rc = replica_check(reps, k, WHAT)) return rc;
        if (!epsnap_like(snaps[k], reps[k]->cfg)) return fail(SMR_ERR_ARG, std::string("epaxos snapshot: made for ") + EPSNAP_OTHER);
        return SMR_OK;
    }
    static int groups_pair_check(smr_ep_replica *const *reps, smr_ep_snapshot *const *snaps, uint32_t k, uint32_t n, SnapGroupsCall call) {
        if (int rc = replica_check(reps, k, GWHAT)) return rc;
        if (call == SNAP_GROUPS_RESET) return SMR_OK;
        if (!epsnap_like_kind(snaps[k], reps[k]->cfg)) return fail(SMR_ERR_ARG, std::string("epaxos groups: the snapshot was made for ") + EPSNAP_OTHER_KIND);
        return snap_groups_len_check(n, snaps[k]->G, GWHAT);
    }
};

// the arguments of the one launch for n replicas and their snapshots (snaps = nullptr: a reset); G: the image's groups -- the
// snapshots' (the whole replica's, or the list's length), not the replicas'
static void epsnap_args(uint32_t n, smr_ep_replica *const *reps, smr_ep_snapshot *const *snaps, uint32_t G, EpSnapArgs &A) {
    memset(&A, 0, sizeof(A));
    const smr_ep_cfg &c0 = reps[0]->cfg;
    A.geo = epsnap_geom(G, c0.population, c0.n_keys, c0.execute, c0.recovery);
    for (uint32_t k = 0; k < n; k++) {
        A.v[k] = reps[k]->v; A.x[k] = reps[k]->x;
        if (!snaps) continue;
        A.img[k] = snaps[k]->buf.dev;
        A.cap_c[k] = snaps[k]->cap[0]; A.cap_r[k] = snaps[k]->cap[1]; A.cap_x[k] = snaps[k]->cap[2]; A.oq[k] = snaps[k]->oq;
    }
}
}  // namespace smr

extern "C" {

int smr_ep_snapshot_create(const smr_ep_replica *like, smr_ep_snapshot **out) { return snap_obj_create<EpSnap>(like, out); }
void smr_ep_snapshot_destroy(smr_ep_snapshot *s) { snap_obj_destroy(s); }

int smr_ep_cluster_save_state(uint32_t n, smr_ep_replica *const *reps, smr_ep_snapshot *const *snaps, void *stream) {
    EpSnapArgs A;
    if (int rc = snap_cluster_setup<EpSnap>(n, reps, snaps, false)) return rc;
    epsnap_args(n, reps, snaps, snaps[0]->G, A);
    hipLaunchKernelGGL(ep_snap_pack, dim3(A.geo.tiles.nblock, n), dim3(256), 0, (hipStream_t)stream, A);
    SMR_HIP_TRY(hipGetLastError());
    for (uint32_t k = 0; k < n; k++) snap_obj_saved(snaps[k]);
    return SMR_OK;
}

int smr_ep_cluster_load_state(uint32_t n, smr_ep_replica *const *reps, const smr_ep_snapshot *const *csnaps, void *stream) {
    smr_ep_snapshot *const *snaps = const_cast<smr_ep_snapshot *const *>(csnaps);   // (a header is read back and cached on first use)
    EpSnapArgs A;
    if (int rc = snap_cluster_setup<EpSnap>(n, reps, snaps, true)) return rc;
    epsnap_args(n, reps, snaps, snaps[0]->G, A);
    hipLaunchKernelGGL(ep_snap_unpack, dim3(A.geo.tiles.nblock, n), dim3(256), 0, (hipStream_t)stream, A);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

// ---- chosen groups between replica objects (ep_snapshot.h: the same image, the same bodies, through a group list) -------------
int smr_ep_snapshot_create_groups(const smr_ep_replica *like, uint32_t n, smr_ep_snapshot **out) { return snap_obj_create_groups<EpSnap>(like, n, out); }

int smr_ep_cluster_save_groups(uint32_t n_reps, smr_ep_replica *const *reps, const uint32_t *groups_host, uint32_t n, smr_ep_snapshot *const *snaps,
                               void *stream) {
    EpSnapArgs A;
    if (int rc = snap_groups_setup<EpSnap>(n_reps, reps, snaps, groups_host, n, SNAP_GROUPS_SAVE)) return rc;
    if (int rc = snap_glist_upload(snaps[0]->glist, groups_host, n, (hipStream_t)stream, EpSnap::GWHAT)) return rc;
    epsnap_args(n_reps, reps, snaps, n, A);
    hipLaunchKernelGGL(ep_snap_pack_groups, dim3(A.geo.tiles.nblock, n_reps), dim3(256), 0, (hipStream_t)stream, A, (const uint32_t *)snaps[0]->glist.dev);
    SMR_HIP_TRY(hipGetLastError());
    for (uint32_t k = 0; k < n_reps; k++) snap_obj_saved(snaps[k]);
    return SMR_OK;
}

int smr_ep_cluster_load_groups(uint32_t n_reps, smr_ep_replica *const *reps, const smr_ep_snapshot *const *csnaps, const uint32_t *groups_host, uint32_t n,
                               void *stream) {
    smr_ep_snapshot *const *snaps = const_cast<smr_ep_snapshot *const *>(csnaps);   // (a header is read back and cached on first use)
    EpSnapArgs A;
    if (int rc = snap_groups_setup<EpSnap>(n_reps, reps, snaps, groups_host, n, SNAP_GROUPS_LOAD)) return rc;
    if (int rc = snap_glist_upload(snaps[0]->glist, groups_host, n, (hipStream_t)stream, EpSnap::GWHAT)) return rc;
    epsnap_args(n_reps, reps, snaps, n, A);
    hipLaunchKernelGGL(ep_snap_unpack_groups, dim3(A.geo.tiles.nblock, n_reps), dim3(256), 0, (hipStream_t)stream, A, (const uint32_t *)snaps[0]->glist.dev, 0);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_ep_cluster_reset_groups(uint32_t n_reps, smr_ep_replica *const *reps, const uint32_t *groups_host, uint32_t n, void *stream) {
    EpSnapArgs A;
    if (int rc = snap_groups_setup<EpSnap>(n_reps, reps, (smr_ep_snapshot *const *)nullptr, groups_host, n, SNAP_GROUPS_RESET)) return rc;
    if (int rc = snap_glist_upload(reps[0]->glist, groups_host, n, (hipStream_t)stream, EpSnap::GWHAT)) return rc;
    epsnap_args(n_reps, reps, nullptr, n, A);
    hipLaunchKernelGGL(ep_snap_unpack_groups, dim3(A.geo.tiles.nblock, n_reps), dim3(256), 0, (hipStream_t)stream, A, (const uint32_t *)reps[0]->glist.dev, 1);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_ep_save_groups(smr_ep_replica *e, const uint32_t *groups_host, uint32_t n, smr_ep_snapshot *s, void *stream) {
    if (!e || !s) return fail(SMR_ERR_ARG, "epaxos groups: null argument");
    return smr_ep_cluster_save_groups(1, &e, groups_host, n, &s, stream);
}

int smr_ep_load_groups(smr_ep_replica *e, const smr_ep_snapshot *s, const uint32_t *groups_host, uint32_t n, void *stream) {
    if (!e || !s) return fail(SMR_ERR_ARG, "epaxos groups: null argument");
    return smr_ep_cluster_load_groups(1, &e, &s, groups_host, n, stream);
}

int smr_ep_reset_groups(smr_ep_replica *e, const uint32_t *groups_host, uint32_t n, void *stream) {
    if (!e) return fail(SMR_ERR_ARG, "epaxos groups: null argument");
    return smr_ep_cluster_reset_groups(1, &e, groups_host, n, stream);
}

int smr_ep_save_state(smr_ep_replica *e, smr_ep_snapshot *s, void *stream) {
    if (!e || !s) return fail(SMR_ERR_ARG, "epaxos snapshot: null argument");
    return smr_ep_cluster_save_state(1, &e, &s, stream);
}

int smr_ep_load_state(smr_ep_replica *e, const smr_ep_snapshot *s, void *stream) {
    if (!e || !s) return fail(SMR_ERR_ARG, "epaxos snapshot: null argument");
    return smr_ep_cluster_load_state(1, &e, &s, stream);
}

int smr_ep_debug_arena_view(smr_ep_replica *e, void **base_dev, uint64_t *n_bytes) {
    if (!e || !base_dev || !n_bytes) return fail(SMR_ERR_ARG, "epaxos: null argument");
    *base_dev = e->arena.base; *n_bytes = e->arena.size;
    return SMR_OK;
}

int smr_ep_snapshot_info_get(const smr_ep_snapshot *cs, smr_ep_snapshot_info *out) {
    if (int rc = snap_obj_info<EpSnap>(cs, out)) return rc;
    const EpSnapHdr &h = cs->hdr;
    out->bytes = h.bytes; out->n_cells = h.n_cells; out->n_exec = h.n_exec;
    out->n_groups = h.n_groups; out->window = h.window; out->n_keys = h.n_keys; out->max_live = h.max_live; out->max_exec = h.max_exec;
    out->population = h.population; out->me = h.me; out->optimized_quorum = h.optimized_quorum; out->execute = h.execute; out->recovery = h.recovery;
    return SMR_OK;
}

int64_t smr_ep_snapshot_export(const smr_ep_snapshot *cs, uint8_t *host, uint64_t cap) { return snap_obj_export<EpSnap>(cs, host, cap); }

int smr_ep_snapshot_import(smr_ep_snapshot *s, const uint8_t *host, uint64_t len) {
    if (!s || !host) return fail(SMR_ERR_ARG, "epaxos snapshot: null argument");
    EpSnapHdr h;
    if (int rc = snap_import_prologue(host, len, EPSNAP_MAGIC, EPSNAP_VERSION, EpSnap::WHAT, h)) return rc;
    if (!epsnap_hdr_like(h, s) || h.reserved0[0] || h.reserved0[1] || h.reserved0[2])
        return fail(SMR_ERR_ARG, std::string("epaxos snapshot: the image is of ") + EPSNAP_OTHER);
    const uint32_t W = h.window, R = s->R, G = s->G, K = s->K;
    if (W < 8 || (W & (W - 1)) || W > EPSNAP_MAX_WINDOW) return fail(SMR_ERR_ARG, "epaxos snapshot: the image's window is not a power of two in 8 .. 2^15");
    const EpSnapGeom q = epsnap_geom_of(s);
    if (snap_truncated(len, q.fixed, h.bytes)) return fail(SMR_ERR_ARG, "epaxos snapshot: truncated image");
    const uint64_t room = h.bytes - q.fixed;                      // the record sections; each count bounded before it is multiplied
    if (h.n_cells > room / sizeof(EpSnapCell) || h.n_replies > room / q.r_stride || h.n_exec > room / sizeof(EpSnapExec) ||
        epsnap_bytes(q, h.n_cells, h.n_replies, h.n_exec) != h.bytes)
        return fail(SMR_ERR_ARG, "epaxos snapshot: the header's counts do not add up to the image's size");
    // the body against the header: counts and maxima recomputed from the scalars, ids in range
    const auto bad = [](const char *what) { return fail(SMR_ERR_ARG, std::string("epaxos snapshot: malformed image: ") + what); };
    const auto u32at = [](const uint8_t *p, uint64_t i) { uint32_t x; memcpy(&x, p + 4 * i, 4); return x; };
    const uint32_t xcap = 2u * R * W;
    uint64_t n_c = 0, n_r = 0, n_x = 0;
    uint32_t max_live = 0, max_exec = 0;
    for (uint32_t g = 0; g < G; g++) {
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t n = ep_live_n(u32at(host + q.o_len, (uint64_t)r * G + g), W);
            if (n > h.max_live) return bad("a row's live span above the header's max_live");
            n_c += n; if (s->recovery || r == s->me) n_r += n;
            max_live = n > max_live ? n : max_live;
        }
        if (host[q.o_rew + g] > 1) return bad("rewritten is neither 0 nor 1");
        const uint32_t nx = s->execute ? u32at(host + q.o_nsub, g) : 0u;
        if (nx > xcap || nx > h.max_exec) return bad("a group's submission list above its capacity or the header's max_exec");
        n_x += nx; max_exec = nx > max_exec ? nx : max_exec;
    }
    if (n_c != h.n_cells || n_r != h.n_replies || n_x != h.n_exec || max_live != h.max_live || max_exec != h.max_exec)
        return bad("the header's counts and maxima contradict the body (the live spans do not sum to n_cells)");
    {
        const uint64_t g = G, rg = 4 * g * R;
        if (!snap_pad_is_zero(host, q.o_len, rg) || !snap_pad_is_zero(host, q.o_cb, rg) || !snap_pad_is_zero(host, q.o_rew, g) ||
            !snap_pad_is_zero(host, q.o_hc, rg * K) ||
            (s->execute && (!snap_pad_is_zero(host, q.o_eb, rg) || !snap_pad_is_zero(host, q.o_pcb, rg) || !snap_pad_is_zero(host, q.o_nsub, 4 * g))))
            return bad("padding is not zero");
        for (uint64_t p = q.o_end; p < q.fixed; p++) if (host[p]) return bad("padding is not zero");
    }
    const uint8_t *p = host + q.fixed;
    for (uint64_t k = 0; k < h.n_cells; k++, p += sizeof(EpSnapCell)) {
        EpSnapCell c;
        memcpy(&c, p, sizeof(c));
        if (c.status > EST_EXECUTED) return bad("an instance's status above Executed");
        if (c.key != EP_NO_KEY && c.key >= K) return bad("an instance's key neither below n_keys nor none");
        for (uint32_t i = R; i < 8; i++) if (c.deps[i] != EP_NONE) return bad("a dependency at or above the population");
        if ((c.pa_acks | c.acc_acks | c.xp_acks | c.xp_has) >> R) return bad("an instance names replicas beyond the population");
        if (!s->recovery && (c.xp_max || c.avoid || c.xp_acks || c.xp_has)) return bad("explicit-prepare fields without recovery");
        if (!(c.bk & 1) && (c.xp_max || c.xp_acks || c.xp_has)) return bad("explicit-prepare bookkeeping of an instance without leader bookkeeping");
    }
    for (uint64_t k = 0; k < h.n_replies; k++, p += q.r_stride) {
        if (s->recovery)
            for (uint32_t i = 0; i < R; i++) {
                if (p[q.r_xs + i] > EST_EXECUTED) return bad("a voted entry's status above Executed");
                if (p[q.r_xk + i] != EP_NO_KEY && p[q.r_xk + i] >= K) return bad("a voted entry's key neither below n_keys nor none");
            }
        for (uint32_t i = q.r_end; i < q.r_stride; i++) if (p[i]) return bad("padding is not zero");
    }
    if (s->execute) {                                            // exec entries, in the image's order (tile, list position, group): a cell of a row
        uint64_t k = 0;
        for (uint32_t t0 = 0; t0 < G; t0 += 64) {
            uint32_t rows = 0;
            for (uint32_t gg = t0; gg < t0 + 64 && gg < G; gg++) { const uint32_t nx = u32at(host + q.o_nsub, gg); rows = nx > rows ? nx : rows; }
            for (uint32_t row = 0; row < rows; row++)
                for (uint32_t gg = t0; gg < t0 + 64 && gg < G; gg++) {
                    if (u32at(host + q.o_nsub, gg) <= row) continue;
                    const uint32_t col = u32at(p, 2 * k), er = u32at(p, 2 * k + 1);
                    k++;
                    if (er >= R || col >= u32at(host + q.o_len, (uint64_t)er * G + gg)) return bad("a submission outside its row");
                }
        }
    }
    return snap_obj_import_bytes<EpSnap>(s, host, h);
}

}  // extern "C"
