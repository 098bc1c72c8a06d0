// Save / load of ONE payload store's state on the device -- the two-plane RSPaxos store and the one-plane CRaft store alike: the
// canonical image and its kernels.  (included by rsp_payload.hip behind PsView)
//
// The store is keyed by ring row plus token (it does not know slots), so the image is keyed by ring row too.  It carries the
// cell headers of every plane the store has, the VOTED plane's alias bytes (observable: a put / ingest into a REQS row takes the
// aliased votes with it, so they are carried, not re-derived), the bytes of every shard that is present and not an alias, and the
// five counters.  It is independent of max_data_len / cap_sl, of the planes' strides and of the store's three allocations.
// Not state, never read and never written: the work list (it_*, flip), dlv (zero between calls), the GF table, row bytes behind
// a shard's length.
//
// Image (little-endian; every section starts on a multiple of 8, the shard bytes on a multiple of 16; padding bytes are zero):
//   PsSnapHdr                                        64 B
//   counters u64[5]                                  copied, rebuilt, unsatisfied, rekeyed, delivered -- summed over their shards
//   per plane p < planes: tok u32[W][G], dlen u32[W][G], avail u8[W][G]   each array padded to 8; where tok is null the rest is zero
//   planes == 2: alias u8[W][G]                      the VOTED cells' shards that live in the REQS row; padded to 8; then zero
//                                                    bytes up to a multiple of 16
//   shard bytes                                      tile-major (64 groups), then plane, ring row, group, and of a cell every shard
//                                                    that is present and not an alias, ascending: ceil(dlen / d) bytes each, zero-
//                                                    padded to a multiple of 16 (the pad is written as zeros, never copied from
//                                                    the row).  An aliased shard's bytes are carried once, in the REQS cell.
// The image is dense: the device buffer holds exactly the exported bytes.
// Chosen groups (smr_rsp_pstore_save_groups / _load_groups / _reset_groups) go through the same image and the same bodies: an
// image of "these n groups, in this order" is the image of an n-group store, read and written through a group list
// (SnapGroupList below): image cell row * n + j is store cell row * G + list[j].  A group image holds zero counters.
#pragma once
#include "snapshot_common.h"

namespace smr {

constexpr uint32_t PSSNAP_MAGIC = 0x42505253u;      // "SRPB"
constexpr uint32_t PSSNAP_VERSION = 1;
constexpr uint32_t PSSNAP_BYTE_BLOCKS = 2048;        // of the byte launch (a grid-stride loop over (cell, shard), a wavefront each)

struct PsSnapHdr {
    uint32_t magic, version, n_groups, window;
    uint8_t n_shards, n_data_shards, planes, craft;
    uint32_t max_dlen;
    uint64_t bytes, n_cells, n_shards_stored, shard_bytes, reserved;
};
static_assert(sizeof(PsSnapHdr) == 64, "image header");

// the one place that knows what a cell contributes to the shard section: its shards that are present and not aliases, each
// ceil(dlen / d) bytes padded to 16 (shared by the kernels and the import's checks)
SMR_HD uint32_t pssnap_shard_len(uint32_t dlen, uint32_t d) { return (dlen + d - 1) / d; }
SMR_HD uint32_t pssnap_stored(uint32_t avail, uint32_t alias) { return avail & ~alias & 0xFFu; }
SMR_HD uint64_t pssnap_cell_bytes(uint32_t stored, uint32_t dlen, uint32_t d) {
    uint32_t n = 0;
    for (uint32_t k = 0; k < 8; k++) n += (stored >> k) & 1u;
    return (uint64_t)n * snap_a16(pssnap_shard_len(dlen, d));
}

struct PsSnapGeom {
    uint32_t G, W, planes;
    SnapTiles tiles;
    uint64_t cells, off_ctr, o_tok[2], o_dlen[2], o_avail[2], o_alias, hdr_end, fixed;
};
SMR_HD PsSnapGeom pssnap_geom(uint32_t G, uint32_t W, uint32_t planes) {
    PsSnapGeom q;
    q.G = G; q.W = W; q.planes = planes; q.tiles = snap_tiles(G);
    q.cells = (uint64_t)G * W;
    q.off_ctr = sizeof(PsSnapHdr);
    uint64_t off = q.off_ctr + 5 * 8;
    for (uint32_t p = 0; p < 2; p++) {
        q.o_tok[p] = off; if (p < planes) off += snap_a8(4 * q.cells);
        q.o_dlen[p] = off; if (p < planes) off += snap_a8(4 * q.cells);
        q.o_avail[p] = off; if (p < planes) off += snap_a8(q.cells);
    }
    q.o_alias = off; if (planes == 2) off += snap_a8(q.cells);
    q.hdr_end = off;
    q.fixed = snap_a16(off);
    return q;
}

// ---- what a new store holds for a group ---------------------------------------------------------------------------------
// The one place that says it: ps_create fills its arrays from here, and smr_rsp_pstore_reset_groups (the unpack of nothing,
// below) returns a listed group's cells to the same values -- every cell's token null, length 0, no shards, no alias.  Row bytes
// are not state where no shard is present and are not touched.
constexpr uint8_t PS_INIT_TOK_BYTE = 0xFF;                   // create fills bytes
constexpr uint32_t PS_INIT_TOK = 0x01010101u * PS_INIT_TOK_BYTE, PS_INIT_WORD = 0;
static_assert(PS_INIT_TOK == PS_NULL && PS_INIT_WORD == 0, "a new cell is a null cell");

// ---- which group of the store an image position holds: snapshot_common.h's SnapAllGroups / SnapGroupList (here the lane
// prefix and cell_off run over list positions too; the positions are always A.geo.G, so the bodies do not ask the map for n) ----
// What a group image does not carry (WHOLE = false): the five counters (zero in the image, the target's left alone).

// ---- the kernels --------------------------------------------------------------------------------------------------------
// Two launches each way, no host read-back between them.
//   (1) ps_snap_head: snapshot_common.h's tiles and bases, summing the groups' byte totals; inside a tile, per
//       (plane, row), a prefix over the 64 lanes gives every cell the offset of its first stored shard (cell_off, a scratch array
//       of the snapshot, not part of the image) -- cells differ in size, so this is a scan where the other images count lanes.
//       The same pass moves the cell headers (canonical) and, from the last tile, writes the image header.
//   (2) ps_snap_bytes: shaped like ps_bytes_kernel -- one wavefront per (cell, shard), one lane per 16-byte column, 16-byte loads
//       and stores on both sides; every byte offset is 64-bit.
struct PsSnapArgs {
    PsView v;
    uint8_t *img;
    uint64_t *cell_off;      // [planes][W][geo.G]: image geometry
    uint64_t cap_bytes;      // room of the shard section
    uint32_t craft;
    PsSnapGeom geo;          // of the image: geo.G = v.G for a whole store, the list's length for chosen groups
};

struct PsSnapCell { uint32_t tok, dlen, avail, alias; };
// a cell of plane P: the store's own at i = row * v.G + g, canonical (PACK), or the image's at i = row * geo.G + x
template <bool PACK, int P>
__device__ __forceinline__ PsSnapCell pssnap_cell(const PsSnapArgs &A, size_t i) {
    PsSnapCell c;
    if (PACK) {
        const PsPlane &pl = A.v.pl[P];
        c.tok = pl.tok[i];
        const bool some = c.tok != PS_NULL;
        c.dlen = some ? pl.dlen[i] : 0u; c.avail = some ? (uint32_t)pl.avail[i] : 0u;
        c.alias = (P == 1 && some && pl.alias) ? ((uint32_t)pl.alias[i] & c.avail) : 0u;
    } else {
        const uint8_t *b = A.img;
        c.tok = ((const uint32_t *)(b + A.geo.o_tok[P]))[i]; c.dlen = ((const uint32_t *)(b + A.geo.o_dlen[P]))[i];
        c.avail = b[A.geo.o_avail[P] + i]; c.alias = P == 1 ? (uint32_t)b[A.geo.o_alias + i] : 0u;
    }
    return c;
}
// what the launch sums over groups: the shard bytes (a cell's offset), and for a save's header the cells with a token, the shards
// stored and (mx[]) the longest payload; a load has those in the image and sums the bytes alone
enum { PS_BYTES = 0, PS_CELLS = 1, PS_SHARDS = 2 };
// (g, G: the group and stride of the side that is read -- the store's for PACK, the image's otherwise)
template <bool PACK, int P>
__device__ __forceinline__ void pssnap_add_group(const PsSnapArgs &A, uint32_t g, size_t G, uint64_t (&sum)[PACK ? 3 : 1], uint32_t (&mx)[1]) {
    for (uint32_t r = 0; r < A.geo.W; r++) {
        const PsSnapCell c = pssnap_cell<PACK, P>(A, (size_t)r * G + g);
        const uint32_t st = pssnap_stored(c.avail, c.alias);
        sum[PS_BYTES] += pssnap_cell_bytes(st, c.dlen, A.v.d);
        if constexpr (PACK) {
            sum[PS_CELLS] += c.tok != PS_NULL ? 1u : 0u; sum[PS_SHARDS] += (uint32_t)__popc(st);
            mx[0] = c.dlen > mx[0] ? c.dlen : mx[0];
        }
    }
}

// one (plane, row) of a tile: the headers across, the cells' offsets from a prefix over the lanes.  xi: the lane's position in the
// image, g: its group in the store.  FRESH (unpack only): no image is read, the cell becomes what ps_create leaves
template <bool PACK, int P, bool FRESH = false>
__device__ __forceinline__ void pssnap_head_row(const PsSnapArgs &A, uint32_t r, uint32_t xi, uint32_t g, bool in, uint32_t lane, uint64_t &run_bytes, uint64_t (&mine)[3], uint32_t (&mine_mx)[1]) {
    const PsSnapGeom &Q = A.geo;
    const size_t i = (size_t)r * Q.G + (in ? xi : 0u), si = (size_t)r * A.v.G + g;
    if constexpr (FRESH) {
        if (in) {
            const PsPlane &pl = A.v.pl[P];
            pl.tok[si] = PS_INIT_TOK; pl.dlen[si] = PS_INIT_WORD; pl.avail[si] = (uint8_t)PS_INIT_WORD;
            if (P == 1 && pl.alias) pl.alias[si] = (uint8_t)PS_INIT_WORD;
        }
        return;
    }
    uint64_t c = 0;
    if (in) {
        const PsSnapCell x = pssnap_cell<PACK, P>(A, PACK ? si : i);
        if (PACK) {
            ((uint32_t *)(A.img + Q.o_tok[P]))[i] = x.tok; ((uint32_t *)(A.img + Q.o_dlen[P]))[i] = x.dlen;
            A.img[Q.o_avail[P] + i] = (uint8_t)x.avail;
            if (P == 1) A.img[Q.o_alias + i] = (uint8_t)x.alias;
        } else {
            const PsPlane &pl = A.v.pl[P];
            pl.tok[si] = x.tok; pl.dlen[si] = x.dlen; pl.avail[si] = (uint8_t)x.avail;
            if (P == 1 && pl.alias) pl.alias[si] = (uint8_t)x.alias;
        }
        const uint32_t st = pssnap_stored(x.avail, x.alias);
        c = pssnap_cell_bytes(st, x.dlen, A.v.d);
        if (PACK) {                                              // (the header's counts: a load has them in the image)
            mine[PS_CELLS] += x.tok != PS_NULL ? 1u : 0u; mine[PS_SHARDS] += (uint32_t)__popc(st);
            mine_mx[0] = x.dlen > mine_mx[0] ? x.dlen : mine_mx[0];
        }
    }
    uint64_t incl = c;
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint64_t y = __shfl(incl, (int)(lane >= off ? lane - off : lane));
        if (lane >= off) incl += y;
    }
    if (in) A.cell_off[((size_t)P * Q.W + r) * Q.G + xi] = run_bytes + (incl - c);
    run_bytes += __shfl(incl, 63);
}

// the head launch of a whole store (ps_snap_head) or of the listed groups (ps_snap_head_groups); tiles are 64 image positions
template <bool PACK, class Map, bool FRESH = false>
__device__ __forceinline__ void pssnap_head_all(const PsSnapArgs &A, const Map &M) {
    const PsSnapGeom &Q = A.geo;
    const PsView &v = A.v;
    const SnapWave w = snap_wave(Q.tiles, Q.G);
    constexpr int NS = PACK ? 3 : 1;
    uint64_t run[NS], mine[3] = {0, 0, 0};                       // in front of this wavefront's tiles; inside them (bytes: in run)
    uint32_t run_mx[1], mine_mx[1] = {0};
    if constexpr (FRESH) run[PS_BYTES] = 0;
    else
        snap_bases(
            [&](uint32_t x, uint64_t (&add)[NS], uint32_t (&m)[1]) {
                const uint32_t g = PACK ? M.group(x, true) : x;
                const size_t G = PACK ? v.G : Q.G;
                pssnap_add_group<PACK, 0>(A, g, G, add, m);
                if (A.geo.planes == 2) pssnap_add_group<PACK, 1>(A, g, G, add, m);
            },
            w.gb0, w.gw0, run, run_mx);
    for (uint32_t t = w.t0; t < w.t1; t++) {
        const uint32_t x = t * 64 + w.lane;
        const bool in = x < Q.G;
        const uint32_t g = M.group(x, in);
        for (uint32_t r = 0; r < Q.W; r++) pssnap_head_row<PACK, 0, FRESH>(A, r, x, g, in, w.lane, run[PS_BYTES], mine, mine_mx);
        if (Q.planes == 2)
            for (uint32_t r = 0; r < Q.W; r++) pssnap_head_row<PACK, 1, FRESH>(A, r, x, g, in, w.lane, run[PS_BYTES], mine, mine_mx);
    }
    if constexpr (PACK) {
        if (Map::WHOLE) snap_counters_save<5>(v.counters, (uint64_t *)(A.img + Q.off_ctr));
        else if (blockIdx.x == 0 && threadIdx.x < 5) ((uint64_t *)(A.img + Q.off_ctr))[threadIdx.x] = 0;   // a group image carries no counters
        if (w.last) {                                            // the wavefront of the last tile knows the totals
            const uint64_t cells = run[PS_CELLS] + snap_wave_sum(mine[PS_CELLS]), shards = run[PS_SHARDS] + snap_wave_sum(mine[PS_SHARDS]);
            const uint32_t mdl = snap_wave_max(mine_mx[0]);
            if (w.lane == 0) {
                PsSnapHdr h;
                h.magic = PSSNAP_MAGIC; h.version = PSSNAP_VERSION; h.n_groups = Q.G; h.window = Q.W;
                h.n_shards = (uint8_t)v.n; h.n_data_shards = (uint8_t)v.d; h.planes = (uint8_t)Q.planes; h.craft = (uint8_t)A.craft;
                h.max_dlen = mdl > run_mx[0] ? mdl : run_mx[0];
                h.n_cells = cells; h.n_shards_stored = shards; h.shard_bytes = run[PS_BYTES];
                h.bytes = Q.fixed + run[PS_BYTES]; h.reserved = 0;
                *(PsSnapHdr *)A.img = h;
                for (uint32_t p = 0; p < Q.planes; p++) {        // padding is zero
                    snap_zero_pad(A.img, Q.o_tok[p], 4 * Q.cells); snap_zero_pad(A.img, Q.o_dlen[p], 4 * Q.cells); snap_zero_pad(A.img, Q.o_avail[p], Q.cells);
                }
                if (Q.planes == 2) snap_zero_pad(A.img, Q.o_alias, Q.cells);
                for (uint64_t b = Q.hdr_end; b < Q.fixed; b++) A.img[b] = 0;     // (up to the shard section's multiple of 16)
            }
        }
    } else if (Map::WHOLE) {
        snap_counters_load<5>((const uint64_t *)(A.img + Q.off_ctr), v.counters);
    }
}
template <bool PACK>
__global__ __launch_bounds__(256) void ps_snap_head(const PsSnapArgs A) { pssnap_head_all<PACK>(A, SnapAllGroups{}); }
// group x of the image (A.geo.G = n groups) <-> group list[x] of the store; fresh (a load only): no image, the listed groups'
// cells as a new store holds them (A carries the geometry of n groups and no buffers)
template <bool PACK>
__global__ __launch_bounds__(256) void ps_snap_head_groups(const PsSnapArgs A, const uint32_t *list, int fresh) {
    if constexpr (PACK) pssnap_head_all<true>(A, SnapGroupList{list});
    else if (fresh) pssnap_head_all<false, SnapGroupList, true>(A, SnapGroupList{list});
    else pssnap_head_all<false>(A, SnapGroupList{list});
}

// the low nb bytes of a word, the rest zero
__device__ __forceinline__ uint32_t pssnap_keep(uint32_t w, uint32_t nb) { return nb >= 4u ? w : (nb ? (w & ((1u << (8u * nb)) - 1u)) : 0u); }

// the byte launch: the image's (plane, cell, shard) items, so chosen groups cost a launch of their own length
template <bool PACK, class Map>
__device__ __forceinline__ void pssnap_bytes_all(const PsSnapArgs &A, const Map &M) {
    const PsSnapGeom &Q = A.geo;
    const PsView &v = A.v;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wv = (uint64_t)blockIdx.x * 4 + SMR_WAVE_UNIFORM(threadIdx.x >> 6), nwv = (uint64_t)gridDim.x * 4;
    const uint64_t items = (uint64_t)Q.planes * Q.cells * v.n;
    for (uint64_t it = wv; it < items; it += nwv) {
        const uint64_t ci64 = it / v.n;                          // plane * cells + cell: up to 2^33 (W x G < 2^32 cells, see ps_create)
        const uint32_t k = (uint32_t)(it - ci64 * v.n);
        const bool p1 = ci64 >= Q.cells;
        const size_t i = (size_t)(ci64 - (p1 ? Q.cells : 0));
        const uint32_t avail = A.img[(p1 ? Q.o_avail[1] : Q.o_avail[0]) + i];
        const uint32_t alias = p1 ? (uint32_t)A.img[Q.o_alias + i] : 0u;
        const uint32_t stored = pssnap_stored(avail, alias);
        if (!((stored >> k) & 1u)) continue;
        const uint32_t dlen = ((const uint32_t *)(A.img + (p1 ? Q.o_dlen[1] : Q.o_dlen[0])))[i];
        const uint32_t sl = pssnap_shard_len(dlen, v.d), sl16 = (uint32_t)snap_a16(sl);
        const uint64_t off = A.cell_off[ci64] + (uint64_t)__popc(stored & ((1u << k) - 1u)) * sl16;
        if (sl16 > v.cap_sl || off + sl16 > A.cap_bytes) continue;                    // (refused by the host / cannot happen)
        const uint32_t row = (uint32_t)(i / Q.G), g = M.group((uint32_t)(i - (size_t)row * Q.G), true);   // (the item is the wavefront's: a uniform load)
        const size_t ro = ps_off(v, row, k, g);                  // 64-bit, in the store's geometry
        uint8_t *const ip = A.img + Q.fixed + off;
        for (uint32_t c0 = lane * 16u; c0 < sl16; c0 += 1024u) {
            if (PACK) {
                // where ps_rd reads a shard whose alias bit is clear: the plane's own row.  (The aliased ones are not read here at
                // all -- stored = avail & ~alias; their bytes are the REQS cell's.  Calling ps_rd itself with a per-wavefront plane
                // put the PsPlane's three pointers into scratch, 24 B: its choice between two fields is a choice between addresses.)
                const uint8_t *const rp = (p1 ? v.pl[1].bytes : v.pl[0].bytes) + ro;
                ps_u32x4 x = ps_load16(rp + c0);
                const uint32_t left = sl - c0;                   // bytes of this column that are the shard's: the rest is written as zeros
                if (left < 16u) {
                    x.x = pssnap_keep(x.x, left); x.y = pssnap_keep(x.y, left > 4u ? left - 4u : 0u);
                    x.z = pssnap_keep(x.z, left > 8u ? left - 8u : 0u); x.w = pssnap_keep(x.w, left > 12u ? left - 12u : 0u);
                }
                ps_store16(ip + c0, x);
            } else {
                uint8_t *rp = (p1 ? v.pl[1].bytes : v.pl[0].bytes) + ro;
                if (c0 + 16u <= sl) ps_store16(rp + c0, ps_load16(ip + c0));
                else for (uint32_t b = c0; b < sl; b++) rp[b] = ip[b];            // bytes behind the shard's length are not the store's state
            }
        }
    }
}
template <bool PACK>
__global__ __launch_bounds__(256) void ps_snap_bytes(const PsSnapArgs A) { pssnap_bytes_all<PACK>(A, SnapAllGroups{}); }
template <bool PACK>
__global__ __launch_bounds__(256) void ps_snap_bytes_groups(const PsSnapArgs A, const uint32_t *list) { pssnap_bytes_all<PACK>(A, SnapGroupList{list}); }

}  // namespace smr
