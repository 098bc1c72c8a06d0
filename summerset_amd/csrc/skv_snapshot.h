// Save / load of the string store's state on the device (smr_skv_*): the canonical image and its kernels.  (included by
// skv_exec.hip behind SkvView)
//
// What the reference's snapshot is first of all -- a dump of the KV pairs (multipaxos/snapshot.rs:14-51 snapshot_dump_kv_pairs,
// :189-260 recover_from_snapshot) -- for G groups at once.  The image holds the live pairs and nothing else: it is independent
// of `slots` and `heap_bytes`, of the probe history and of the bytes overwritten Puts left behind in the heap, so two stores
// that hold the same maps export the same bytes, and an image loaded back is a compaction of the heap.
//
// Image (little-endian; every section starts on a multiple of 8, the byte section on a multiple of 16; padding bytes are zero
// and are written as zeros, never copied from a heap):
//   SkvSnapHdr                                       64 B
//   n_keys u32[n]                                    padded to 8
//   full   u8[n]                                     0 / 1, the sticky flag (it travels: a frozen group stays frozen); padded to 8
//   records {hash u64, klen u32, vlen u32}           16 B each; then zero bytes up to a multiple of 16
//   bytes                                            per record, in record order: the key bytes, then the value bytes, the
//                                                    record's run zero-padded to a multiple of 16 (klen + vlen == 0: no bytes).
//                                                    Offsets are not stored: they follow from the records in front (64-bit)
// Record order: tile-major over 64 image positions, then rank k, then position (what snap_place produces).  Rank within a group:
// ascending (hash, klen, key bytes), hash being the stored FNV-1a word of the key.
// On the device the two record sections sit at fixed capacities behind the fixed part; export closes the gaps.
//
// Load, deterministic in (image, slots), per listed group: the table cleared (klen = SKV_EMPTY, every other field 0), the
// records inserted in rank order by linear probing from hash & mask, each record's key and then its value written contiguously
// in record order from heap offset 0.  Afterwards heap_used = sum(klen + vlen); heap bytes at and behind it are not state and are
// not touched.
//
// Chosen groups (smr_skv_save_groups / _load_groups / _reset_groups) go through the same image and the same bodies: an image of
// "these n groups, in this order" is the image of an n-group store, read and written through a group list (SnapGroupList).
#pragma once
#include "snapshot_common.h"

namespace smr {

constexpr uint32_t SKVSNAP_MAGIC = 0x564B5353u;      // "SSKV"
constexpr uint32_t SKVSNAP_VERSION = 1;
constexpr uint32_t SKVSNAP_BYTE_BLOCKS = 2048;       // of the byte launch (a grid-stride loop over records, a wavefront each)
constexpr uint32_t SKVSNAP_RANK_BLOCKS = 4096;       // of the rank launch (a grid-stride loop over image positions, a wavefront each)

struct SkvSnapHdr {
    uint32_t magic, version, n_groups, max_keys;
    uint32_t max_group_bytes, reserved0;             // max over groups of sum(klen + vlen), unpadded
    uint64_t bytes, n_records, byte_bytes, reserved[2];
};
static_assert(sizeof(SkvSnapHdr) == 64, "image header");

struct SkvSnapRec { uint64_t hash; uint32_t klen, vlen; };
static_assert(sizeof(SkvSnapRec) == 16, "image record");

// ---- what a new store holds for a group ---------------------------------------------------------------------------------
// The one place that says it: smr_skv_create fills its arrays from here, and smr_skv_reset_groups (the unpack of nothing)
// returns a listed group to the same values -- every entry free, every other entry field 0, an empty heap, not full.  Heap bytes
// are not state and are not touched.
constexpr uint8_t SKV_INIT_KLEN_BYTE = 0xFF;                 // create fills bytes
constexpr uint32_t SKV_INIT_KLEN = 0x01010101u * SKV_INIT_KLEN_BYTE, SKV_INIT_WORD = 0;
static_assert(SKV_INIT_KLEN == SKV_EMPTY && SKV_INIT_WORD == 0, "a new entry is a free entry");

SMR_HD uint64_t skvsnap_fnv1a(const uint8_t *p, uint32_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint32_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001B3ull; }
    return h;
}

// the image of n groups: the fixed part; the sections behind it depend on the counts (packed) or the capacities (device)
struct SkvSnapGeom {
    uint32_t G;
    SnapTiles tiles;
    uint64_t o_nkeys, o_full, fixed;                 // fixed: the end of the fixed part = the records' offset in the packed image
};
SMR_HD SkvSnapGeom skvsnap_geom(uint32_t G) {
    SkvSnapGeom q;
    q.G = G; q.tiles = snap_tiles(G);
    q.o_nkeys = sizeof(SkvSnapHdr);
    q.o_full = q.o_nkeys + snap_a8(4 * (uint64_t)G);
    q.fixed = q.o_full + snap_a8(G);
    return q;
}
// packed image: where the byte section starts behind n_records records, and the image's size
SMR_HD uint64_t skvsnap_bytes_at(const SkvSnapGeom &q, uint64_t n_records) { return snap_a16(q.fixed + 16 * n_records); }
// device buffer: records at a multiple of 16 behind the fixed part, the byte section behind room for cap_rec records
SMR_HD uint64_t skvsnap_dev_rec(const SkvSnapGeom &q) { return snap_a16(q.fixed); }
SMR_HD uint64_t skvsnap_dev_bytes(const SkvSnapGeom &q, uint64_t cap_rec) { return skvsnap_dev_rec(q) + 16 * cap_rec; }

// scratch of the launches, owned by the snapshot, not part of the image: the rank pass's results per image position (which
// slot holds rank k, the live entries, their padded and unpadded byte totals) and per record where its bytes lie on both sides
struct SkvSnapSrc { uint32_t g, koff, voff, pad; };          // the store's side of a record: group, key and value offsets in its strip
struct SkvSnapScratch {
    uint32_t *order;         // [slots][geo.G]: the slot of the entry of rank k
    uint32_t *cnt;           // [geo.G]
    uint32_t *graw;          // [geo.G]
    uint64_t *gbytes;        // [geo.G]
    uint64_t *rec_off;       // [cap_rec]: the record's offset in the byte section
    SkvSnapSrc *src;         // [cap_rec]
};
SMR_HD uint64_t skvsnap_scratch_layout(uint32_t G, uint32_t slots, uint64_t cap_rec, uint8_t *base, SkvSnapScratch *out) {
    uint64_t off = 0;
    const uint64_t o_order = off; off += snap_a16(4 * (uint64_t)slots * G);
    const uint64_t o_cnt = off; off += snap_a16(4 * (uint64_t)G);
    const uint64_t o_raw = off; off += snap_a16(4 * (uint64_t)G);
    const uint64_t o_gb = off; off += snap_a16(8 * (uint64_t)G);
    const uint64_t o_ro = off; off += snap_a16(8 * cap_rec);
    const uint64_t o_src = off; off += 16 * cap_rec;
    if (out) {
        out->order = (uint32_t *)(base + o_order); out->cnt = (uint32_t *)(base + o_cnt); out->graw = (uint32_t *)(base + o_raw);
        out->gbytes = (uint64_t *)(base + o_gb); out->rec_off = (uint64_t *)(base + o_ro); out->src = (SkvSnapSrc *)(base + o_src);
    }
    return off + 16;
}

struct SkvSnapArgs {
    SkvView v;
    uint8_t *img;
    SkvSnapScratch sc;
    uint64_t cap_rec, cap_bytes;     // room of the two record sections
    uint64_t n_records;              // a load: the header's (the host has it); a save: unused, the byte launch reads the header
    SkvSnapGeom geo;                 // of the image: geo.G = v.G for a whole store, the list's length for chosen groups
};

// ---- the kernels --------------------------------------------------------------------------------------------------------
// Three launches each way, no host read-back between them.
//   (1) the sizes in front.  Save -- skv_snap_rank: a wavefront per image position ranks the group's live entries by counting
//       (lane = slot, 64 slots a chunk; the other entries' hashes come across the wavefront, O(live * slots / 64) steps) and leaves
//       order[k][x], the live count and the group's byte totals.  Load -- skv_snap_head<SIZES>: the groups' padded byte totals
//       out of the image's records.
//   (2) skv_snap_head: snapshot_common.h's tiles and bases over the per-group counts of (1); inside a tile, per rank, a prefix
//       over the 64 lanes gives every record its offset in the byte section (records differ in size: a scan, as in
//       ps_snapshot.h).  The same pass moves the records (a load: clears the table and inserts them) and, from the last tile,
//       writes the image header.
//   (3) skv_snap_bytes: one wavefront per record, one lane per 16-byte column of the record's run.  The image side is 16-byte
//       aligned; the heap side is byte-granular (koff / voff are arbitrary).  Every byte offset is 64-bit.

// entry a < entry b of group g where their hashes are equal: (klen, key bytes).  Two live entries never hold the same key
__device__ __forceinline__ bool skvsnap_key_less(const SkvView &v, uint32_t g, uint32_t a, uint32_t b) {
    const size_t ea = (size_t)a * v.G + g, eb = (size_t)b * v.G + g;
    const uint32_t la = v.klen[ea], lb = v.klen[eb];
    if (la != lb) return la < lb;
    const uint64_t oa = v.koff[ea], ob = v.koff[eb];
    if (oa + la > v.heap_bytes || ob + lb > v.heap_bytes) return a < b;       // (cannot happen)
    const uint8_t *const heap = v.heap + (size_t)g * v.heap_bytes;
    for (uint32_t i = 0; i < la; i++) {
        const uint8_t x = heap[oa + i], y = heap[ob + i];
        if (x != y) return x < y;
    }
    return a < b;                                                              // (cannot happen: the same key twice)
}

template <class Map>
__device__ __forceinline__ void skvsnap_rank_all(const SkvSnapArgs &A, const Map &M) {
    const SkvView &v = A.v;
    const uint32_t lane = threadIdx.x & 63u, n = A.geo.G;
    const uint32_t wv = blockIdx.x * 4 + SMR_WAVE_UNIFORM(threadIdx.x >> 6), nwv = gridDim.x * 4;
    const uint32_t nch = (v.slots + 63) / 64;
    for (uint32_t x = wv; x < n; x += nwv) {
        const uint32_t g = M.group(x, true);
        uint64_t cnt = 0, gb = 0, raw = 0;
        for (uint32_t ci = 0; ci < nch; ci++) {
            const uint32_t s = ci * 64 + lane;
            bool live = false;
            uint64_t h = 0;
            uint32_t kl = 0, vl = 0;
            if (s < v.slots) {
                const size_t e = (size_t)s * v.G + g;
                kl = v.klen[e];
                live = kl != SKV_EMPTY;
                if (live) { h = v.hash[e]; vl = v.vlen[e]; }
            }
            if (!__ballot(live)) continue;                                     // (the wavefront's: no lane of this chunk has an entry)
            uint32_t r = 0;
            for (uint32_t cj = 0; cj < nch; cj++) {
                const uint32_t t = cj * 64 + lane;
                bool lj = live;
                uint64_t hj = h;
                if (cj != ci) {
                    lj = false; hj = 0;
                    if (t < v.slots) {
                        const size_t e = (size_t)t * v.G + g;
                        lj = v.klen[e] != SKV_EMPTY;
                        if (lj) hj = v.hash[e];
                    }
                }
                unsigned long long m = __ballot(lj);
                while (m) {                                                    // the chunk's live entries, one after the other
                    const int l = __ffsll(m) - 1;
                    m &= m - 1;
                    const uint64_t ho = __shfl(hj, l);
                    const uint32_t so = cj * 64 + (uint32_t)l;
                    if (live && so != s && (ho < h || (ho == h && skvsnap_key_less(v, g, so, s)))) r++;
                }
            }
            if (live) {
                if (r < v.slots) A.sc.order[(size_t)r * n + x] = s;
                const uint64_t len = (uint64_t)kl + vl;
                cnt++; gb += snap_a16(len); raw += len;
            }
        }
        cnt = snap_wave_sum(cnt); gb = snap_wave_sum(gb); raw = snap_wave_sum(raw);
        if (lane == 0) {
            A.sc.cnt[x] = (uint32_t)cnt; A.sc.gbytes[x] = gb;
            A.sc.graw[x] = raw > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)raw;
        }
    }
}
__global__ __launch_bounds__(256) void skv_snap_rank(const SkvSnapArgs A) { skvsnap_rank_all(A, SnapAllGroups{}); }
__global__ __launch_bounds__(256) void skv_snap_rank_groups(const SkvSnapArgs A, const uint32_t *list) { skvsnap_rank_all(A, SnapGroupList{list}); }

// what smr_skv_create leaves for group g
__device__ __forceinline__ void skvsnap_group_init(const SkvView &v, uint32_t g) {
    for (uint32_t s = 0; s < v.slots; s++) {
        const size_t e = (size_t)s * v.G + g;
        v.hash[e] = SKV_INIT_WORD; v.koff[e] = SKV_INIT_WORD; v.klen[e] = SKV_INIT_KLEN; v.voff[e] = SKV_INIT_WORD; v.vlen[e] = SKV_INIT_WORD;
    }
    v.heap_used[g] = SKV_INIT_WORD; v.n_keys[g] = SKV_INIT_WORD; v.full[g] = (uint8_t)SKV_INIT_WORD;
}

enum { SKVSNAP_PACK = 0, SKVSNAP_UNPACK = 1, SKVSNAP_SIZES = 2, SKVSNAP_FRESH = 3 };
enum { SKV_RECS = 0, SKV_BYTES = 1 };

// the head launch of a whole store or of the listed groups; tiles are 64 image positions.  SIZES (a load's first launch): only
// gbytes[x] out of the image; FRESH (a reset): no image, the listed groups as a new store holds them
template <int MODE, class Map>
__device__ __forceinline__ void skvsnap_head_all(const SkvSnapArgs &A, const Map &M) {
    const SkvSnapGeom &Q = A.geo;
    const SkvView &v = A.v;
    const SnapWave w = snap_wave(Q.tiles, Q.G);
    if constexpr (MODE == SKVSNAP_FRESH) {
        for (uint32_t t = w.t0; t < w.t1; t++) {
            const uint32_t x = t * 64 + w.lane;
            if (x < Q.G) skvsnap_group_init(v, M.group(x, true));
        }
        return;
    } else {
        constexpr bool PACK = MODE == SKVSNAP_PACK, SIZES = MODE == SKVSNAP_SIZES;
        const uint32_t *const cnt_of = PACK ? A.sc.cnt : (const uint32_t *)(A.img + Q.o_nkeys);
        const uint32_t cnt_max = PACK ? v.slots : 0xFFFFFFFFu;
        const SkvSnapRec *const recs = (const SkvSnapRec *)(A.img + skvsnap_dev_rec(Q));
        SkvSnapRec *const recs_w = (SkvSnapRec *)(A.img + skvsnap_dev_rec(Q));
        const uint64_t n_rec = PACK ? A.cap_rec : (A.n_records < A.cap_rec ? A.n_records : A.cap_rec);
        uint64_t run[2];
        uint32_t run_mx[2], mine_keys = 0, mine_raw = 0;
        snap_bases(
            [&](uint32_t x, uint64_t (&add)[2], uint32_t (&m)[2]) {
                const uint32_t c = cnt_of[x];
                add[SKV_RECS] += c; m[0] = c > m[0] ? c : m[0];
                if constexpr (!SIZES) add[SKV_BYTES] += A.sc.gbytes[x];
                if constexpr (PACK) { const uint32_t r = A.sc.graw[x]; m[1] = r > m[1] ? r : m[1]; }
            },
            w.gb0, w.gw0, run, run_mx);
        for (uint32_t t = w.t0; t < w.t1; t++) {
            const uint32_t x = t * 64 + w.lane;
            const bool in = x < Q.G;
            const uint32_t g = SIZES ? 0u : M.group(x, in);
            uint32_t c = in ? cnt_of[x] : 0u;
            c = c < cnt_max ? c : cnt_max;
            if constexpr (MODE == SKVSNAP_UNPACK) {
                c = c < v.slots ? c : v.slots;                               // (the host has checked max_keys <= slots)
                if (in) skvsnap_group_init(v, g);
            }
            if constexpr (PACK) {
                if (in) { ((uint32_t *)(A.img + Q.o_nkeys))[x] = c; A.img[Q.o_full + x] = v.full[g] ? 1 : 0; }
            }
            uint64_t mine_bytes = 0;                                         // this group's: padded (SIZES), in its heap (UNPACK), unpadded (PACK)
            const uint32_t rows = snap_wave_max(c);
            mine_keys = rows > mine_keys ? rows : mine_keys;
            for (uint32_t k = 0; k < rows; k++) {
                const bool act = k < c;
                const unsigned long long mask = __ballot(act);
                const uint64_t pos = run[SKV_RECS] + (uint64_t)__popcll(mask & ((1ull << w.lane) - 1ull));
                const bool ok = act && pos < n_rec;
                SkvSnapRec rec = {0, 0, 0};
                uint32_t ko = 0, vo = 0;
                if (ok) {
                    if constexpr (PACK) {
                        const uint32_t s = A.sc.order[(size_t)k * Q.G + x];
                        if (s < v.slots) {
                            const size_t e = (size_t)s * v.G + g;
                            rec.hash = v.hash[e]; rec.klen = v.klen[e]; rec.vlen = v.vlen[e]; ko = v.koff[e]; vo = v.voff[e];
                        }
                    } else {
                        rec = recs[pos];
                    }
                }
                const uint64_t len = (uint64_t)rec.klen + rec.vlen, l16 = snap_a16(len);
                if constexpr (SIZES) {
                    mine_bytes += l16;
                } else {
                    uint64_t incl = l16;
                    for (uint32_t off = 1; off < 64; off <<= 1) {
                        const uint64_t y = __shfl(incl, (int)(w.lane >= off ? w.lane - off : w.lane));
                        if (w.lane >= off) incl += y;
                    }
                    if (ok) {
                        if constexpr (PACK) {
                            recs_w[pos] = rec;
                            mine_bytes += len;
                        } else {                                             // insert: linear probing from hash & mask, the bytes behind the group's last
                            uint32_t s = (uint32_t)rec.hash & v.mask, probe = 0;
                            for (; probe < v.slots && v.klen[(size_t)s * v.G + g] != SKV_EMPTY; probe++) s = (s + 1) & v.mask;
                            ko = (uint32_t)mine_bytes; vo = ko + rec.klen;
                            if (probe < v.slots && mine_bytes + len <= v.heap_bytes) {   // (the host has checked max_group_bytes <= heap_bytes)
                                const size_t e = (size_t)s * v.G + g;
                                v.hash[e] = rec.hash; v.koff[e] = ko; v.klen[e] = rec.klen; v.voff[e] = vo; v.vlen[e] = rec.vlen;
                                mine_bytes += len;
                            } else {
                                ko = vo = 0xFFFFFFFFu;                       // (no bytes for the byte launch to move)
                            }
                        }
                        A.sc.rec_off[pos] = run[SKV_BYTES] + (incl - l16);
                        A.sc.src[pos] = SkvSnapSrc{g, ko, vo, 0u};
                    }
                    run[SKV_BYTES] += __shfl(incl, 63);
                }
                run[SKV_RECS] += (uint64_t)__popcll(mask);
            }
            if constexpr (SIZES) {
                if (in) A.sc.gbytes[x] = mine_bytes;
            }
            if constexpr (MODE == SKVSNAP_UNPACK) {
                if (in) { v.heap_used[g] = (uint32_t)mine_bytes; v.n_keys[g] = c; v.full[g] = A.img[Q.o_full + x] ? 1 : 0; }
            }
            if constexpr (PACK) {
                const uint32_t r = mine_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)mine_bytes;
                mine_raw = r > mine_raw ? r : mine_raw;
            }
        }
        if constexpr (PACK) {
            if (w.last) {                                                    // the wavefront of the last tile knows the totals
                const uint32_t raw = snap_wave_max(mine_raw);
                if (w.lane == 0) {
                    SkvSnapHdr h;
                    h.magic = SKVSNAP_MAGIC; h.version = SKVSNAP_VERSION; h.n_groups = Q.G;
                    h.max_keys = mine_keys > run_mx[0] ? mine_keys : run_mx[0];
                    h.max_group_bytes = raw > run_mx[1] ? raw : run_mx[1]; h.reserved0 = 0;
                    h.n_records = run[SKV_RECS]; h.byte_bytes = run[SKV_BYTES];
                    h.bytes = skvsnap_bytes_at(Q, h.n_records) + h.byte_bytes;
                    h.reserved[0] = h.reserved[1] = 0;
                    *(SkvSnapHdr *)A.img = h;
                    snap_zero_pad(A.img, Q.o_nkeys, 4 * (uint64_t)Q.G); snap_zero_pad(A.img, Q.o_full, Q.G);   // padding is zero
                }
            }
        }
    }
}
template <int MODE>
__global__ __launch_bounds__(256) void skv_snap_head(const SkvSnapArgs A) { skvsnap_head_all<MODE>(A, SnapAllGroups{}); }
// group x of the image (A.geo.G = n groups) <-> group list[x] of the store
template <int MODE>
__global__ __launch_bounds__(256) void skv_snap_head_groups(const SkvSnapArgs A, const uint32_t *list) { skvsnap_head_all<MODE>(A, SnapGroupList{list}); }

struct alignas(16) SkvSnapCol { uint32_t w[4]; };           // a 16-byte column of a record's run, as the image holds it
__device__ __forceinline__ void skvsnap_col_put(SkvSnapCol &c, uint32_t i, uint32_t byte) { c.w[i >> 2] |= byte << (8u * (i & 3u)); }
__device__ __forceinline__ uint8_t skvsnap_col_get(const SkvSnapCol &c, uint32_t i) { return (uint8_t)(c.w[i >> 2] >> (8u * (i & 3u))); }

// the byte launch: the image's records; where a record's bytes lie in the store is in src[] (the head launch has been through
// the group map), so a whole store and chosen groups run the same kernel
template <bool PACK>
__global__ __launch_bounds__(256) void skv_snap_bytes(const SkvSnapArgs A) {
    const SkvSnapGeom &Q = A.geo;
    const SkvView &v = A.v;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wv = (uint64_t)blockIdx.x * 4 + SMR_WAVE_UNIFORM(threadIdx.x >> 6), nwv = (uint64_t)gridDim.x * 4;
    uint64_t n_rec = PACK ? ((const SkvSnapHdr *)A.img)->n_records : A.n_records;
    n_rec = n_rec < A.cap_rec ? n_rec : A.cap_rec;
    const SkvSnapRec *const recs = (const SkvSnapRec *)(A.img + skvsnap_dev_rec(Q));
    uint8_t *const bytes = A.img + skvsnap_dev_bytes(Q, A.cap_rec);
    for (uint64_t r = wv; r < n_rec; r += nwv) {
        const SkvSnapRec rec = recs[r];
        const SkvSnapSrc src = A.sc.src[r];
        const uint64_t off = A.sc.rec_off[r];
        const uint64_t kl = rec.klen, len = kl + rec.vlen, l16 = snap_a16(len);
        if (off + l16 > A.cap_bytes || src.g >= v.G) continue;                                       // (cannot happen)
        if ((uint64_t)src.koff + kl > v.heap_bytes || (uint64_t)src.voff + rec.vlen > v.heap_bytes) continue;   // (refused by the host / cannot happen)
        uint8_t *const heap = v.heap + (size_t)src.g * v.heap_bytes;                                 // 64-bit: g * heap_bytes passes 4 GiB
        uint8_t *const kp = heap + src.koff, *const vp = heap + src.voff;
        uint8_t *const ip = bytes + off;
        for (uint64_t c0 = (uint64_t)lane * 16u; c0 < l16; c0 += 1024u) {
            SkvSnapCol col = {{0, 0, 0, 0}};
            if (PACK) {
                if (c0 + 16u <= kl) memcpy(col.w, kp + c0, 16);                                       // the whole column out of one run: no alignment assumed
                else if (c0 >= kl && c0 + 16u <= len) memcpy(col.w, vp + (c0 - kl), 16);
                else {
#pragma unroll
                    for (uint32_t i = 0; i < 16u; i++) {                                             // across the key's end or the record's: the pad is written as zeros
                        const uint64_t b = c0 + i;
                        if (b < len) skvsnap_col_put(col, i, b < kl ? kp[b] : vp[b - kl]);
                    }
                }
                *(SkvSnapCol *)(ip + c0) = col;
            } else {
                col = *(const SkvSnapCol *)(ip + c0);
                if (c0 + 16u <= kl) memcpy(kp + c0, col.w, 16);
                else if (c0 >= kl && c0 + 16u <= len) memcpy(vp + (c0 - kl), col.w, 16);
                else {
#pragma unroll
                    for (uint32_t i = 0; i < 16u; i++) {                                             // bytes behind the record's length are not the store's state
                        const uint64_t b = c0 + i;
                        if (b < kl) kp[b] = skvsnap_col_get(col, i);
                        else if (b < len) vp[b - kl] = skvsnap_col_get(col, i);
                    }
                }
            }
        }
    }
}

}  // namespace smr
