// What the five device-resident snapshots (mp_snapshot.h, raft_snapshot.h, rsp_snapshot.h, ps_snapshot.h, ep_snapshot.h) have in common: how a
// launch is cut into tiles, how a record finds its place in an image, the sharded counters, and the host's handling of the device
// buffer and of an image's outer checks.  The formats and the field moves stay with the engines.
//
// The scheme.  Lane = group, a wavefront = a contiguous piece of the 64-group tiles, 4 wavefronts a block.  A record's place in its
// section follows from the counts of everything in front of it: the block sums the groups in front of its own tiles itself (a few
// bytes per group out of the L2: no block waits for another), the wavefront adds the tiles of its block in front of its own
// (snap_bases), and inside a tile a row's records go to the lanes that hold one, packed (snap_place: ballot + prefix count) -- a
// wavefront's stores of a row are one contiguous piece.  The wavefront of the last tile ends up knowing the totals and writes the
// header.  On the device the record sections sit at fixed capacities behind the fixed part; export closes the gaps.
#pragma once
#include <string.h>

#include <initializer_list>
#include <vector>

#include "smr_common.h"

#ifndef SMR_HD
#if defined(__HIPCC__)
#define SMR_HD __host__ __device__ __forceinline__
#else
#define SMR_HD inline
#endif
#endif

namespace smr {

SMR_HD uint64_t snap_a8(uint64_t x) { return (x + 7) & ~(uint64_t)7; }
SMR_HD uint64_t snap_a16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// ---- the tile partition ---------------------------------------------------------------------------------------------------
constexpr uint32_t SNAP_MAX_WAVES = 1024;          // wavefronts of a launch (per replica); each takes a contiguous piece of the group tiles
struct SnapTiles { uint32_t ntile, tpw, nwave, nblock; };   // 64-group tiles, tiles per wavefront, wavefronts, blocks of 4 wavefronts
SMR_HD SnapTiles snap_tiles(uint32_t G) {
    SnapTiles t;
    t.ntile = (G + 63) / 64;
    t.tpw = (t.ntile + SNAP_MAX_WAVES - 1) / SNAP_MAX_WAVES;
    t.nwave = (t.ntile + t.tpw - 1) / t.tpw;
    t.nblock = (t.nwave + 3) / 4;
    return t;
}

// ---- device ---------------------------------------------------------------------------------------------------------------
// wave-wide reductions (all 64 lanes must be active)
__device__ __forceinline__ uint64_t snap_wave_sum(uint64_t x) {
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ uint32_t snap_wave_max(uint32_t x) {
    for (int off = 32; off > 0; off >>= 1) { uint32_t y = __shfl_xor(x, off); x = y > x ? y : x; }
    return x;
}

// this wavefront's share of a launch over G groups: its tiles [t0, t1), the first group of its block's tiles and of its own
// (both clamped to G), and whether it holds the last tile (that wavefront knows the totals)
struct SnapWave { uint32_t lane, t0, t1, gb0, gw0; bool last; };
__device__ __forceinline__ SnapWave snap_wave(const SnapTiles &T, uint32_t G) {
    const uint32_t lane = threadIdx.x & 63u, wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t tb0 = blockIdx.x * 4 * T.tpw, t0 = wv * T.tpw;
    const uint32_t t1 = t0 + T.tpw < T.ntile ? t0 + T.tpw : T.ntile;
    const uint32_t gb0 = tb0 * 64 < G ? tb0 * 64 : G, gw0 = t0 * 64 < G ? t0 * 64 : G;
    return SnapWave{lane, t0, t1, gb0, gw0, t0 < T.ntile && t1 == T.ntile};
}

// sums and maxima over the groups [0, gw0); gb0 <= gw0 is the same for the whole block (256 threads, every one of them calls).
// count(g, add, mx) adds group g's counts to add[NSUM] and raises mx[NMAX]; the sums are integers, so the order does not matter
template <int NSUM, int NMAX, class Count>
__device__ __forceinline__ void snap_bases(const Count &count, uint32_t gb0, uint32_t gw0, uint64_t (&sum)[NSUM], uint32_t (&mx)[NMAX]) {
    __shared__ uint64_t sh_s[NSUM][4];
    __shared__ uint32_t sh_m[NMAX][4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t s[NSUM];
    uint32_t m[NMAX];
#pragma unroll
    for (int k = 0; k < NSUM; k++) s[k] = 0;
#pragma unroll
    for (int k = 0; k < NMAX; k++) m[k] = 0;
    for (uint32_t g = threadIdx.x; g < gb0; g += 256) count(g, s, m);
#pragma unroll
    for (int k = 0; k < NSUM; k++) s[k] = snap_wave_sum(s[k]);
#pragma unroll
    for (int k = 0; k < NMAX; k++) m[k] = snap_wave_max(m[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NSUM; k++) sh_s[k][w] = s[k];
#pragma unroll
        for (int k = 0; k < NMAX; k++) sh_m[k][w] = m[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NSUM; k++) { sum[k] = sh_s[k][0] + sh_s[k][1] + sh_s[k][2] + sh_s[k][3]; s[k] = 0; }
#pragma unroll
    for (int k = 0; k < NMAX; k++) {
        mx[k] = sh_m[k][0];
#pragma unroll
        for (int j = 1; j < 4; j++) mx[k] = sh_m[k][j] > mx[k] ? sh_m[k][j] : mx[k];
        m[k] = 0;
    }
    for (uint32_t g = gb0 + lane; g < gw0; g += 64) count(g, s, m);
#pragma unroll
    for (int k = 0; k < NSUM; k++) sum[k] += snap_wave_sum(s[k]);
#pragma unroll
    for (int k = 0; k < NMAX; k++) { const uint32_t x = snap_wave_max(m[k]); mx[k] = x > mx[k] ? x : mx[k]; }
}

// the rows of one tile: this lane's group holds n records, `base` is the section index of the tile's first one on entry and of
// the next tile's on return.  Row k goes to the lanes with k < n, packed; body(k, pos) runs for those of them with pos < cap.
// Returns the tile's longest row count (the header's max_* fields)
template <class Body>
__device__ __forceinline__ uint32_t snap_place(uint32_t n, uint64_t &base, uint64_t cap, uint32_t lane, const Body &body) {
    const uint32_t rows = snap_wave_max(n);
    for (uint32_t k = 0; k < rows; k++) {
        const bool act = k < n;
        const unsigned long long mask = __ballot(act);
        const uint64_t pos = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (act && pos < cap) body(k, pos);
        base += (uint64_t)__popcll(mask);
    }
    return rows;
}

// the first N event counters (smr_common.h: SMR_CTR_SHARDS partial sums each).  Save: the shards summed, by wave 0 of block 0;
// load: the sums into shard 0, the other shards (and the words behind N) zero, by block 0.  Every thread of the launch calls.
// Ctr: the engine's pointer to its counters (MultiPaxos types it as global address space)
template <int N, class Ctr>
__device__ __forceinline__ void snap_counters_save(Ctr counters, uint64_t *dst) {
    static_assert(N <= (int)SMR_CTR_STRIDE, "counters of one shard");
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    unsigned long long x[N];
#pragma unroll
    for (int k = 0; k < N; k++) x[k] = 0;
    for (uint32_t sh = threadIdx.x; sh < SMR_CTR_SHARDS; sh += 64) {
#pragma unroll
        for (int k = 0; k < N; k++) x[k] += counters[(size_t)sh * SMR_CTR_STRIDE + k];
    }
#pragma unroll
    for (int k = 0; k < N; k++) x[k] = snap_wave_sum(x[k]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) dst[k] = x[k];
    }
}
template <int N, class Ctr>
__device__ __forceinline__ void snap_counters_load(const uint64_t *src, Ctr counters) {
    static_assert(SMR_CTR_SHARDS == 256 && N <= (int)SMR_CTR_STRIDE, "one thread of block 0 per counter shard");
    if (blockIdx.x != 0) return;
    for (uint32_t k = 0; k < SMR_CTR_STRIDE; k++) counters[(size_t)threadIdx.x * SMR_CTR_STRIDE + k] = (threadIdx.x == 0 && k < N) ? src[k] : 0ull;
}

// padding is zero: the bytes between the n an array at `off` (a multiple of 8) holds and the next multiple of 8
__device__ __forceinline__ void snap_zero_pad(uint8_t *base, uint64_t off, uint64_t n) {
    for (uint64_t p = off + n; p < off + snap_a8(n); p++) base[p] = 0;
}

// ---- which group of the object an image position holds --------------------------------------------------------------------
// An image has its own group index (position x, stride n = its n_groups, lane = x & 63) and the engine object has its own
// (group g, stride = its n_groups).  For a whole-object image they are one and the same; an image of "these n groups, in this
// order" (the save_groups / load_groups calls) is the image of an n-group object whose group x is group list[x] of this one:
// the same format, the same tiles, bases and placement run over list positions, and the object's side a gather or scatter
// (two listed groups share a line of a ring row only where they sit in the same 64-group tile).  The engines' pack and unpack
// bodies take the map as a parameter, so the field moves are written once; with SnapAllGroups they are the whole-object
// kernels.  WHOLE = false: the object's reporting (its counters, ...) does not travel -- events stay counted where they
// happened, so the sum over objects is conserved; each engine's header says what that is for its image.
// n(G_obj, G_img): the positions of the image, out of the object's and the image geometry's group counts; group(x, in): `in`
// is false for the lanes behind the last position
struct SnapAllGroups {
    static constexpr bool WHOLE = true;
    __device__ __forceinline__ uint32_t n(uint32_t G_obj, uint32_t) const { return G_obj; }
    __device__ __forceinline__ uint32_t group(uint32_t x, bool) const { return x; }
};
struct SnapGroupList {
    static constexpr bool WHOLE = false;
    const uint32_t *__restrict__ list;                           // [n], every entry < G_obj, none twice (the host has checked)
    __device__ __forceinline__ uint32_t n(uint32_t, uint32_t G_img) const { return G_img; }
    __device__ __forceinline__ uint32_t group(uint32_t x, bool in) const { return in ? list[x] : 0u; }
};

// ---- host -----------------------------------------------------------------------------------------------------------------
// `what` is the engine's message prefix ("raft snapshot: ", ...): every text below is what the engines said before they shared it.

// a snapshot object's device buffer: `filled` once a save or import has run, `hdr_known` once the image's header is on the host
struct SnapBuf {
    int device = -1;                                             // (where the engine keeps track of it)
    uint8_t *dev = nullptr;
    bool filled = false, hdr_known = false;
};
inline int snap_buf_alloc(SnapBuf &b, uint64_t bytes, const char *what) {
    if (b.dev) { SMR_HIP_TRY(hipDeviceSynchronize()); (void)hipFree(b.dev); b.dev = nullptr; }
    hipError_t e = hipMalloc((void **)&b.dev, bytes);
    if (e != hipSuccess) { b.dev = nullptr; return fail(SMR_ERR_DEVICE, std::string(what) + "hipMalloc: " + hipGetErrorString(e)); }
    return SMR_OK;
}
inline void snap_buf_free(SnapBuf &b) {
    if (b.dev) { (void)hipDeviceSynchronize(); (void)hipFree(b.dev); b.dev = nullptr; }
}
// the image's header on the host (synchronises once after a save); fits(hdr): its counts are within the buffer's capacities
template <class Hdr, class Fits>
int snap_buf_header(SnapBuf &b, Hdr &hdr, const char *what, const Fits &fits) {
    if (!b.filled) return fail(SMR_ERR_STATE, std::string(what) + "nothing saved or imported yet");
    if (b.hdr_known) return SMR_OK;
    SMR_HIP_TRY(hipDeviceSynchronize());
    SMR_HIP_TRY(hipMemcpy(&hdr, b.dev, sizeof(Hdr), hipMemcpyDeviceToHost));
    if (!fits(hdr)) {                                            // (cannot happen: the kernels' counts are bounded by what the room was made for)
        b.filled = false;
        return fail(SMR_ERR_STATE, std::string(what) + "the saved state exceeds the snapshot's room");
    }
    b.hdr_known = true;
    return SMR_OK;
}

// a record section: `bytes` at dev_off on the device (capacity-spaced), `pad_to` >= bytes in the packed image, the rest zero.
// The fixed part and then every section, device to packed host image (export: to_host, the padding written) or back (import)
struct SnapSection { uint64_t dev_off, bytes, pad_to; };
inline int snap_copy_sections(uint8_t *dev, uint8_t *host, uint64_t fixed, bool to_host, std::initializer_list<SnapSection> secs) {
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    SMR_HIP_TRY(hipMemcpy(to_host ? host : dev, to_host ? dev : host, fixed, kind));
    uint8_t *p = host + fixed;
    for (const SnapSection &s : secs) {
        if (s.bytes) SMR_HIP_TRY(hipMemcpy(to_host ? p : dev + s.dev_off, to_host ? dev + s.dev_off : p, s.bytes, kind));
        if (to_host) memset(p + s.bytes, 0, s.pad_to - s.bytes);
        p += s.pad_to;
    }
    return SMR_OK;
}

// an import's first checks: length, magic, version; the header copied out.  noun: what the magic message calls the image
template <class Hdr>
int snap_import_prologue(const uint8_t *host, uint64_t len, uint32_t magic, uint32_t version, const char *what, Hdr &h, const char *noun = "snapshot") {
    if (len < sizeof(Hdr)) return fail(SMR_ERR_ARG, std::string(what) + "image shorter than its header");
    memcpy(&h, host, sizeof(h));
    if (h.magic != magic) return fail(SMR_ERR_ARG, std::string(what) + "not a " + noun + " image (magic)");
    if (h.version != version)
        return fail(SMR_ERR_ARG, std::string(what) + "image format version " + std::to_string(h.version) + ", this library reads " + std::to_string(version));
    return SMR_OK;
}
// len bytes cannot hold an image of `bytes` with a fixed part of `fixed`
inline bool snap_truncated(uint64_t len, uint64_t fixed, uint64_t bytes) { return len < fixed || bytes > len || bytes < fixed; }
inline bool snap_pad_is_zero(const uint8_t *host, uint64_t off, uint64_t n) {
    for (uint64_t p = off + n; p < off + snap_a8(n); p++) if (host[p]) return false;
    return true;
}

// the cluster forms' lists: n replicas and their snapshots, nothing null, nothing listed twice; each(k) is the engine's own
// comparison of pair k (against reps[0], snapshot against replica), run in the same pass so the first fault found is the one
// the engines reported before they shared this
template <class Rep, class Snap, class Each>
int snap_pairs_check(uint32_t n, Rep *const *reps, Snap *const *snaps, const char *what, const Each &each) {
    if (!reps || !snaps) return fail(SMR_ERR_ARG, std::string(what) + "null argument");
    if (n == 0 || n > SMR_MAX_REPLICAS) return fail(SMR_ERR_ARG, std::string(what) + "1 .. 8 replicas");
    for (uint32_t k = 0; k < n; k++) {
        if (!reps[k] || !snaps[k]) return fail(SMR_ERR_ARG, std::string(what) + "null argument");
        for (uint32_t j = 0; j < k; j++)
            if (reps[j] == reps[k] || snaps[j] == snaps[k]) return fail(SMR_ERR_ARG, std::string(what) + "a replica or a snapshot is listed twice");
        if (int rc = each(k)) return rc;
    }
    return SMR_OK;
}

// a list of groups for a listed-groups call (chosen groups between objects: the list is a host array -- a move is a rare host
// decision -- checked before anything is launched).  On the device it lives in a buffer owned by the snapshot object the call
// works on (a reset: by the engine object), made once and grown only when a longer list comes
struct SnapGroupListBuf { uint32_t *dev = nullptr; uint32_t cap = 0; };
inline int snap_glist_room(SnapGroupListBuf &b, uint32_t n, const char *what) {
    if (b.dev && n <= b.cap) return SMR_OK;
    if (b.dev) { SMR_HIP_TRY(hipDeviceSynchronize()); (void)hipFree(b.dev); b.dev = nullptr; b.cap = 0; }   // (a launch may still read it)
    hipError_t e = hipMalloc((void **)&b.dev, (size_t)n * 4);
    if (e != hipSuccess) { b.dev = nullptr; return fail(SMR_ERR_DEVICE, std::string(what) + "hipMalloc of the list: " + hipGetErrorString(e)); }
    b.cap = n;
    return SMR_OK;
}
inline void snap_glist_free(SnapGroupListBuf &b) {
    if (b.dev) { (void)hipDeviceSynchronize(); (void)hipFree(b.dev); b.dev = nullptr; b.cap = 0; }
}
// n in 1 .. G, every id below G, none twice (a bitmap: O(n)).  of: what the first message calls the G ("a cluster of ", or nothing)
inline int snap_glist_check(const uint32_t *groups, uint32_t n, uint32_t G, const char *what, const char *of = "") {
    if (n == 0 || n > G) return fail(SMR_ERR_ARG, std::string(what) + "a list of " + std::to_string(n) + " groups for " + of + std::to_string(G));
    std::vector<uint64_t> seen(((size_t)G + 63) / 64, 0ull);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t g = groups[i];
        if (g >= G) return fail(SMR_ERR_ARG, std::string(what) + "list entry " + std::to_string(i) + " is group " + std::to_string(g) + " of " + std::to_string(G));
        if ((seen[g >> 6] >> (g & 63u)) & 1ull) return fail(SMR_ERR_ARG, std::string(what) + "group " + std::to_string(g) + " is listed twice");
        seen[g >> 6] |= 1ull << (g & 63u);
    }
    return SMR_OK;
}
// The list in front of the kernel, on its stream.  The caller's array is pageable memory, which the runtime has read (staged)
// by the time the copy call returns: the caller may reuse it at once, and the next call may overwrite the device buffer, in
// stream order
inline int snap_glist_upload(SnapGroupListBuf &b, const uint32_t *groups, uint32_t n, hipStream_t st, const char *what) {
    if (int rc = snap_glist_room(b, n, what)) return rc;
    SMR_HIP_TRY(hipMemcpyAsync(b.dev, groups, (size_t)n * 4, hipMemcpyHostToDevice, st));
    return SMR_OK;
}

// ---- host: one snapshot object, one call path ----------------------------------------------------------------
// An engine's snapshot struct derives from SnapObj and adds what it was made for (G = its n_groups, and the engine's own
// fields); a struct E of static members says what is the engine's own.  S = the snapshot struct, Like = the engine object:
//   WHAT, GWHAT, NOUN          message prefixes of the whole-object and the listed-groups calls; what the engine object is called
//   LIST_FIRST, LIST_OF        listed-groups calls: the list is checked before the pairs (MultiPaxos), and what it calls G
//   groups_of(like)            the engine object's n_groups
//   init(s, like)              s's own fields from `like` (s->G is set); may refuse, may allocate s->scratch
//   need(s, like, n[N])        the sections' worst case for s's groups in an object like `like`
//   counts(hdr, n[N])          the header's section counts
//   dev_bytes(s)               the device buffer for s->cap
//   copy(s, host, hdr, to_host)   the image between the device buffer and packed host bytes
//   load_fits(s, like, what, groups)   a load's rules on s->hdr: the image is of s's kind, and fits `like` (window, ...)
//   pair_check(reps, snaps, k)         the whole-object cluster calls' check of pair k
//   groups_pair_check(reps, snaps, k, n, call)   the listed-groups calls' (snaps = nullptr for a reset)
template <class Hdr, int N>
struct SnapObj {
    static constexpr int NSEC = N;
    SnapBuf buf;
    uint64_t cap[N] = {};                                        // records (the stores: bytes) the device buffer's sections have room for
    Hdr hdr;                                                     // the image's header, once buf.hdr_known
    SnapGroupListBuf glist;                                      // the save_groups / load_groups calls' list on the device
    void *scratch = nullptr;                                     // device memory of the launches that is not image (the stores' cell_off)
};

// room for `need` records per section: grows (host-known sizes: no read-back), and what the buffer held goes with the old one
template <class E, class S>
int snap_obj_room(S *s, const uint64_t (&need)[S::NSEC]) {
    bool fits = s->buf.dev != nullptr;
    for (int k = 0; k < S::NSEC; k++) fits = fits && need[k] <= s->cap[k];
    if (fits) return SMR_OK;
    s->buf.filled = false; s->buf.hdr_known = false;
    for (int k = 0; k < S::NSEC; k++) s->cap[k] = need[k] > s->cap[k] ? need[k] : s->cap[k];
    return snap_buf_alloc(s->buf, E::dev_bytes(s), E::WHAT);
}
// ... for the worst case of s's groups in an object like `like`: a save can then never find the snapshot too small, so it stays
// a call that only enqueues
template <class E, class S, class Like>
int snap_obj_room_for(S *s, const Like *like) {
    uint64_t need[S::NSEC];
    E::need(s, like, need);
    return snap_obj_room<E>(s, need);
}
// the image's header on the host (synchronises once after a save)
template <class E, class S>
int snap_obj_header(S *s) {
    return snap_buf_header(s->buf, s->hdr, E::WHAT, [s](const decltype(s->hdr) &h) {
        uint64_t n[S::NSEC];
        E::counts(h, n);
        for (int k = 0; k < S::NSEC; k++) if (n[k] > s->cap[k]) return false;
        return true;
    });
}
template <class S>
void snap_obj_saved(S *s) { s->buf.filled = true; s->buf.hdr_known = false; }
// before a load writes anything: the header, and the engine's rules on it
template <class E, class S, class Like>
int snap_obj_load_ready(S *s, const Like *like, const char *what, bool groups) {
    if (int rc = snap_obj_header<E>(s)) return rc;
    return E::load_fits(s, like, what, groups);
}

// every device buffer of the object synchronises before it is freed: a launch may still use it
template <class S>
void snap_obj_destroy(S *s) {
    if (!s) return;
    snap_buf_free(s->buf);
    snap_glist_free(s->glist);
    if (s->scratch) { (void)hipDeviceSynchronize(); (void)hipFree(s->scratch); }
    delete s;
}
// a snapshot object for n groups of an object like `like` (n = its n_groups: the whole object)
template <class E, class S, class Like>
int snap_obj_make(const Like *like, uint32_t n, S **out) {
    S *s = new S();
    s->G = n;
    memset(&s->hdr, 0, sizeof(s->hdr));
    int rc = E::init(s, like);
    if (rc == SMR_OK) rc = snap_obj_room_for<E>(s, like);
    if (rc != SMR_OK) { snap_obj_destroy(s); return rc; }
    *out = s;
    return SMR_OK;
}
template <class E, class S, class Like>
int snap_obj_create(const Like *like, S **out) {
    if (!like || !out) return fail(SMR_ERR_ARG, std::string(E::WHAT) + "null argument");
    return snap_obj_make<E>(like, E::groups_of(like), out);
}
template <class E, class S, class Like>
int snap_obj_create_groups(const Like *like, uint32_t n, S **out) {
    if (!like || !out) return fail(SMR_ERR_ARG, std::string(E::GWHAT) + "null argument");
    if (n == 0 || n > E::groups_of(like))
        return fail(SMR_ERR_ARG, std::string(E::GWHAT) + "a snapshot of " + std::to_string(n) + " groups of a " + E::NOUN + " of " + std::to_string(E::groups_of(like)));
    S *s = nullptr;
    if (int rc = snap_obj_make<E>(like, n, &s)) return rc;
    if (int rc = snap_glist_room(s->glist, n, E::GWHAT)) { snap_obj_destroy(s); return rc; }   // no allocation in the calls that use it
    *out = s;
    return SMR_OK;
}

// info_get's first half: the header on the host, *out zeroed; the engine copies the fields
template <class E, class S, class Info>
int snap_obj_info(const S *cs, Info *out) {
    if (!cs || !out) return fail(SMR_ERR_ARG, std::string(E::WHAT) + "null argument");
    if (int rc = snap_obj_header<E>(const_cast<S *>(cs))) return rc;
    memset(out, 0, sizeof(*out));
    return SMR_OK;
}
template <class E, class S>
int64_t snap_obj_export(const S *cs, uint8_t *host, uint64_t cap) {
    if (!cs || !host) return fail(SMR_ERR_ARG, std::string(E::WHAT) + "null argument");
    S *s = const_cast<S *>(cs);
    if (int rc = snap_obj_header<E>(s)) return rc;
    if (cap < s->hdr.bytes) return fail(SMR_ERR_ARG, std::string(E::WHAT) + "the image takes " + std::to_string(s->hdr.bytes) + " bytes");
    if (int rc = E::copy(s, host, s->hdr, true)) return rc;
    return (int64_t)s->hdr.bytes;
}
// an import's last step, once the engine has validated the image of header h: room, then the bytes
template <class E, class S, class Hdr>
int snap_obj_import_bytes(S *s, const uint8_t *host, const Hdr &h) {
    uint64_t n[S::NSEC];
    E::counts(h, n);
    if (int rc = snap_obj_room<E>(s, n)) return rc;
    SMR_HIP_TRY(hipDeviceSynchronize());
    s->buf.filled = false;
    if (int rc = E::copy(s, const_cast<uint8_t *>(host), h, false)) return rc;
    s->hdr = h; s->buf.filled = true; s->buf.hdr_known = true;
    return SMR_OK;
}

// the whole-object cluster calls (n replicas and their snapshots): every check before anything is written, then room for a save.
// The engine fills its launch arguments afterwards
template <class E, class Rep, class S>
int snap_cluster_setup(uint32_t n, Rep *const *reps, S *const *snaps, bool load) {
    if (int rc = snap_pairs_check(n, reps, snaps, E::WHAT, [&](uint32_t k) { return E::pair_check(reps, snaps, k); })) return rc;
    for (uint32_t k = 0; k < n; k++)                             // (a save: only a failed hipMalloc -- the snapshots that grew before it are
        if (int rc = load ? snap_obj_load_ready<E>(snaps[k], reps[k], E::WHAT, false) : snap_obj_room_for<E>(snaps[k], reps[k])) return rc;   // then empty, none holds a partial image)
    return SMR_OK;
}

// the listed-groups calls over n_reps objects (the one-object engines: 1) for the n listed groups, one list for all of them:
// every check before anything is written, allocated or launched, in the order the engine's messages have always come; then the
// headers and fit rules of a load, room for a save.  A reset has no snapshots: the objects stand in for them in the pairs' check
enum SnapGroupsCall { SNAP_GROUPS_SAVE, SNAP_GROUPS_LOAD, SNAP_GROUPS_RESET };
inline int snap_groups_len_check(uint32_t n, uint32_t G_snap, const char *what) {
    if (G_snap != n) return fail(SMR_ERR_ARG, std::string(what) + "a list of " + std::to_string(n) + " groups and a snapshot made for " + std::to_string(G_snap));
    return SMR_OK;
}
template <class E, class Rep, class S>
int snap_groups_setup(uint32_t n_reps, Rep *const *reps, S *const *snaps, const uint32_t *groups, uint32_t n, SnapGroupsCall call) {
    if (!groups) return fail(SMR_ERR_ARG, std::string(E::GWHAT) + "null argument");
    const auto list = [&] { return snap_glist_check(groups, n, E::groups_of(reps[0]), E::GWHAT, E::LIST_OF); };
    const auto pair = [&](uint32_t k) {
        if (E::LIST_FIRST && k == 0)
            if (int rc = list()) return rc;
        return E::groups_pair_check(reps, snaps, k, n, call);
    };
    if (int rc = call == SNAP_GROUPS_RESET ? snap_pairs_check(n_reps, reps, reps, E::GWHAT, pair) : snap_pairs_check(n_reps, reps, snaps, E::GWHAT, pair)) return rc;
    if (!E::LIST_FIRST)
        if (int rc = list()) return rc;
    for (uint32_t k = 0; k < n_reps && call != SNAP_GROUPS_RESET; k++)
        if (int rc = call == SNAP_GROUPS_LOAD ? snap_obj_load_ready<E>(snaps[k], reps[k], E::GWHAT, true) : snap_obj_room_for<E>(snaps[k], reps[k])) return rc;
    return SMR_OK;
}

}  // namespace smr
