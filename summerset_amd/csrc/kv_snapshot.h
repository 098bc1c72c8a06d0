// Save / load of the token table's state on the device (smr_kv_*): the image and its one kernel.  (included by kv_exec.hip
// behind KvView)
//
// The table kv[K][G] is all the state there is (keys < K, a value is a 32-bit token, 0 = None), so the image is the table:
//   KvSnapHdr                                        64 B
//   kv u32[K][n]                                     padded to 8 (zero bytes)
// little-endian, dense: the device buffer holds exactly the exported bytes.  Chosen groups (smr_kv_save_groups / _load_groups /
// _reset_groups) go through the same image and the same body: an image of "these n groups, in this order" is the image of an
// n-group table, read and written through a group list (SnapGroupList): image cell k * n + x is table cell k * G + list[x].
#pragma once
#include "snapshot_common.h"

namespace smr {

constexpr uint32_t KVSNAP_MAGIC = 0x564B4B53u;       // "SKKV"
constexpr uint32_t KVSNAP_VERSION = 1;
constexpr uint32_t KVSNAP_BLOCKS = 2048;             // of the launch (a grid-stride loop over the image's cells)

struct KvSnapHdr {
    uint32_t magic, version, n_groups, n_keys;
    uint64_t bytes, reserved[5];
};
static_assert(sizeof(KvSnapHdr) == 64, "image header");

// what a new table holds: the one place that says it -- smr_kv_create fills from here, smr_kv_reset_groups (the unpack of
// nothing) returns a listed group's cells to it
constexpr uint32_t KV_INIT_TOKEN = 0;                // None

SMR_HD uint64_t kvsnap_cells(uint32_t G, uint32_t K) { return (uint64_t)G * K; }
SMR_HD uint64_t kvsnap_bytes(uint32_t G, uint32_t K) { return sizeof(KvSnapHdr) + snap_a8(4 * kvsnap_cells(G, K)); }

struct KvSnapArgs {
    KvView v;
    uint8_t *img;
    uint64_t cap_cells;      // room of the cell section
    uint32_t n;              // of the image: v.G for a whole table, the list's length for chosen groups
};

enum { KVSNAP_PACK = 0, KVSNAP_UNPACK = 1, KVSNAP_FRESH = 2 };

// one pass over the image's cells, a thread each: consecutive threads are consecutive positions of one key's row, so the image
// side is contiguous and the table side is for a whole table too (for a list: a gather or scatter)
template <int MODE, class Map>
__device__ __forceinline__ void kvsnap_all(const KvSnapArgs &A, const Map &M) {
    const KvView &v = A.v;
    const uint64_t cells = kvsnap_cells(A.n, v.K), step = (uint64_t)gridDim.x * 256;
    uint32_t *const img = (uint32_t *)(A.img + sizeof(KvSnapHdr));
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += step) {
        const uint32_t k = (uint32_t)(i / A.n), x = (uint32_t)(i - (uint64_t)k * A.n);
        const size_t c = (size_t)k * v.G + M.group(x, true);
        if (MODE == KVSNAP_FRESH) v.kv[c] = KV_INIT_TOKEN;
        else if (i < A.cap_cells) {
            if (MODE == KVSNAP_PACK) img[i] = v.kv[c];
            else v.kv[c] = img[i];
        }
    }
    if (MODE == KVSNAP_PACK && blockIdx.x == 0 && threadIdx.x == 0) {
        KvSnapHdr h;
        h.magic = KVSNAP_MAGIC; h.version = KVSNAP_VERSION; h.n_groups = A.n; h.n_keys = v.K;
        h.bytes = kvsnap_bytes(A.n, v.K);
        for (int j = 0; j < 5; j++) h.reserved[j] = 0;
        *(KvSnapHdr *)A.img = h;
        if (cells <= A.cap_cells) snap_zero_pad(A.img, sizeof(KvSnapHdr), 4 * cells);               // padding is zero
    }
}
template <int MODE>
__global__ __launch_bounds__(256) void kv_snap(const KvSnapArgs A) { kvsnap_all<MODE>(A, SnapAllGroups{}); }
template <int MODE>
__global__ __launch_bounds__(256) void kv_snap_groups(const KvSnapArgs A, const uint32_t *list) { kvsnap_all<MODE>(A, SnapGroupList{list}); }

}  // namespace smr
