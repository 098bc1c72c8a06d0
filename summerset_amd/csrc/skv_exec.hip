// Device-resident KV state machine over REAL keys and values (VERDICT r1 "missing" #5):
// `StateMachineExecutorTask::execute` (src/server/statemach.rs:193-202) on `State = HashMap<String, String>`
// (:21-63) for G independent groups, lane = group, commands applied row after row in submission order.
//
// Per group: an open-addressing table of `slots` entries (linear probing on a 64-bit FNV-1a hash of the key bytes;
// an entry = hash, key (off, len) and value (off, len) into the group's heap) and an append-only byte heap holding
// the key and value bytes a Put brought.  A Put of an existing key appends the new value and repoints the entry;
// the old bytes stay where they are, so the (off, len) a result names -- Get { value }, Put { old_value } -- remains
// readable for as long as the object lives (no compaction).  Commands name their bytes by (off, len) into a payload
// buffer of the caller (the decoded ReqBatch bytes, already on the device).  Entry fields are SoA [slots][G]: a
// wavefront probing the same slot index touches one contiguous run per field; the heaps are per-group strips.
// A table or heap that runs full sets the group's sticky `full` flag; its later commands answer as no-ops (state 2).
#include <string.h>

#include "smr_common.h"

namespace smr {

constexpr uint32_t SKV_EMPTY = 0xFFFFFFFFu;

struct SkvView {
    uint32_t G, slots, mask;
    uint64_t heap_bytes;
    uint64_t *hash;                 // [slots][G]
    uint32_t *koff, *klen, *voff, *vlen;   // [slots][G]; klen == SKV_EMPTY: free entry
    uint8_t *heap;                  // [G][heap_bytes]
    uint32_t *heap_used;            // [G]
    uint8_t *full;                  // [G]
    uint32_t *n_keys;               // [G]
};

__device__ __forceinline__ uint64_t fnv1a(const uint8_t *p, uint32_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint32_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001B3ull; }
    return h;
}
__device__ __forceinline__ bool bytes_eq(const uint8_t *a, const uint8_t *b, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) if (a[i] != b[i]) return false;
    return true;
}

// kind[n_rows][G]: 0 Get, 1 Put, else no command.  res_state: 0 = None, 1 = Some (res_off / res_len into the group's
// heap), 2 = refused (group full).  Get: value; Put: old_value.
__global__ __launch_bounds__(256) void skv_execute_kernel(const SkvView v, uint32_t n_rows, const uint8_t *__restrict__ kind,
                                                          const uint8_t *__restrict__ payload, uint64_t payload_bytes,
                                                          const uint32_t *__restrict__ key_off, const uint32_t *__restrict__ key_len,
                                                          const uint32_t *__restrict__ val_off, const uint32_t *__restrict__ val_len,
                                                          uint8_t *__restrict__ res_state, uint32_t *__restrict__ res_off,
                                                          uint32_t *__restrict__ res_len) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= v.G) return;
    uint8_t *const heap = v.heap + (size_t)g * v.heap_bytes;
    uint32_t used = v.heap_used[g], nk = v.n_keys[g];
    bool full = v.full[g] != 0;
    for (uint32_t i = 0; i < n_rows; i++) {
        const size_t o = (size_t)i * v.G + g;
        const uint32_t kd = kind[o];
        uint8_t st = 0; uint32_t ro = 0, rl = 0;
        if (kd <= 1) {
            const uint32_t ko = key_off[o], kl = key_len[o];
            const uint32_t vo = kd == 1 ? val_off[o] : 0u, vl = kd == 1 ? val_len[o] : 0u;
            const bool in_buf = (uint64_t)ko + kl <= payload_bytes && (uint64_t)vo + vl <= payload_bytes && kl != SKV_EMPTY;
            if (full || !in_buf) st = 2;
            else {
                const uint8_t *kp = payload + ko;
                const uint64_t h = fnv1a(kp, kl);
                uint32_t s = (uint32_t)h & v.mask;
                bool found = false, free_slot = false;
                for (uint32_t probe = 0; probe < v.slots; probe++, s = (s + 1) & v.mask) {
                    const size_t e = (size_t)s * v.G + g;
                    const uint32_t el = v.klen[e];
                    if (el == SKV_EMPTY) { free_slot = true; break; }
                    if (el == kl && v.hash[e] == h && bytes_eq(heap + v.koff[e], kp, kl)) { found = true; break; }
                }
                const size_t e = (size_t)s * v.G + g;
                if (found) { st = 1; ro = v.voff[e]; rl = v.vlen[e]; }          // state.get(key) / what insert() returns
                if (kd == 1) {                                                  // state.insert(key, value)
                    const uint64_t need = (uint64_t)vl + (found ? 0u : kl);
                    if ((!found && !free_slot) || (uint64_t)used + need > v.heap_bytes) { full = true; st = 2; ro = rl = 0; }
                    else {
                        if (!found) {
                            for (uint32_t b = 0; b < kl; b++) heap[used + b] = kp[b];
                            v.hash[e] = h; v.koff[e] = used; v.klen[e] = kl;
                            used += kl; nk++;
                        }
                        const uint8_t *vp = payload + vo;
                        for (uint32_t b = 0; b < vl; b++) heap[used + b] = vp[b];
                        v.voff[e] = used; v.vlen[e] = vl;
                        used += vl;
                    }
                }
            }
        }
        res_state[o] = st; res_off[o] = ro; res_len[o] = rl;
    }
    v.heap_used[g] = used; v.n_keys[g] = nk;
    if (full) v.full[g] = 1;
}

}  // namespace smr

#include "skv_snapshot.h"

using namespace smr;

struct smr_skv {
    SkvView v; Arena arena;
    SnapGroupListBuf glist;   // smr_skv_reset_groups' list on the device
};

extern "C" {

int smr_skv_create(uint32_t n_groups, uint32_t slots, uint64_t heap_bytes, smr_skv **out) {
    if (!out || !n_groups) return fail(SMR_ERR_ARG, "skv: n_groups is zero");
    if (slots < 2 || (slots & (slots - 1))) return fail(SMR_ERR_ARG, "skv: slots must be a power of two >= 2");
    if (heap_bytes == 0 || heap_bytes > 0xFFFFFFFFull) return fail(SMR_ERR_ARG, "skv: heap_bytes must be in 1 .. 2^32 - 1");
    smr_skv *h = new smr_skv();
    SkvView &v = h->v;
    v.G = n_groups; v.slots = slots; v.mask = slots - 1; v.heap_bytes = heap_bytes;
    const size_t G = n_groups, SG = (size_t)slots * G;
    Arena &a = h->arena;
    const size_t o_h = a.reserve(SG * 8), o_ko = a.reserve(SG * 4), o_kl = a.reserve(SG * 4), o_vo = a.reserve(SG * 4), o_vl = a.reserve(SG * 4),
                 o_hp = a.reserve(G * heap_bytes), o_u = a.reserve(G * 4), o_f = a.reserve(G), o_n = a.reserve(G * 4);
    a.size = a.used;
    hipError_t e = hipMalloc((void **)&a.base, a.size);
    // a group's initial values are skv_snapshot.h's SKV_INIT_* (shared with smr_skv_reset_groups)
    if (e == hipSuccess) e = hipMemset(a.base, (int)SKV_INIT_WORD, a.size);
    if (e == hipSuccess) e = hipMemset(a.base + o_kl, SKV_INIT_KLEN_BYTE, SG * 4);          // every entry free
    if (e != hipSuccess) { if (a.base) (void)hipFree(a.base); delete h; return fail(SMR_ERR_DEVICE, std::string("skv: alloc: ") + hipGetErrorString(e)); }
    v.hash = a.at<uint64_t>(o_h); v.koff = a.at<uint32_t>(o_ko); v.klen = a.at<uint32_t>(o_kl); v.voff = a.at<uint32_t>(o_vo);
    v.vlen = a.at<uint32_t>(o_vl); v.heap = a.at<uint8_t>(o_hp); v.heap_used = a.at<uint32_t>(o_u); v.full = a.at<uint8_t>(o_f);
    v.n_keys = a.at<uint32_t>(o_n);
    *out = h;
    return SMR_OK;
}

void smr_skv_destroy(smr_skv *h) {
    if (!h) return;
    (void)hipDeviceSynchronize();
    snap_glist_free(h->glist);
    if (h->arena.base) (void)hipFree(h->arena.base);
    delete h;
}

int smr_skv_execute(smr_skv *h, uint32_t n_rows, const uint8_t *kind_dev, const uint8_t *payload_dev, uint64_t payload_bytes,
                    const uint32_t *key_off_dev, const uint32_t *key_len_dev, const uint32_t *val_off_dev, const uint32_t *val_len_dev,
                    uint8_t *res_state_dev, uint32_t *res_off_dev, uint32_t *res_len_dev, void *stream) {
    if (!h || !kind_dev || !key_off_dev || !key_len_dev || !val_off_dev || !val_len_dev || !res_state_dev || !res_off_dev || !res_len_dev ||
        (!payload_dev && payload_bytes))
        return fail(SMR_ERR_ARG, "skv: null argument");
    if (!n_rows) return SMR_OK;
    hipLaunchKernelGGL(skv_execute_kernel, dim3((h->v.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->v, n_rows, kind_dev, payload_dev,
                       payload_bytes, key_off_dev, key_len_dev, val_off_dev, val_len_dev, res_state_dev, res_off_dev, res_len_dev);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_skv_heap(smr_skv *h, uint8_t **heap_dev, uint64_t *heap_bytes_per_group) {
    if (!h || !heap_dev) return fail(SMR_ERR_ARG, "skv: null argument");
    *heap_dev = h->v.heap;
    if (heap_bytes_per_group) *heap_bytes_per_group = h->v.heap_bytes;
    return SMR_OK;
}

int smr_skv_read(smr_skv *h, uint32_t group, uint32_t off, uint32_t len, uint8_t *host_buf) {
    if (!h || (!host_buf && len)) return fail(SMR_ERR_ARG, "skv: null argument");
    if (group >= h->v.G || (uint64_t)off + len > h->v.heap_bytes) return fail(SMR_ERR_ARG, "skv: bytes outside the group's heap");
    SMR_HIP_TRY(hipDeviceSynchronize());
    if (len) SMR_HIP_TRY(hipMemcpy(host_buf, h->v.heap + (size_t)group * h->v.heap_bytes + off, len, hipMemcpyDeviceToHost));
    return SMR_OK;
}

int smr_skv_stats(smr_skv *h, uint32_t *n_keys_host, uint32_t *heap_used_host, uint8_t *full_host) {
    if (!h || !n_keys_host || !heap_used_host || !full_host) return fail(SMR_ERR_ARG, "skv: null argument");
    SMR_HIP_TRY(hipDeviceSynchronize());
    SMR_HIP_TRY(hipMemcpy(n_keys_host, h->v.n_keys, (size_t)h->v.G * 4, hipMemcpyDeviceToHost));
    SMR_HIP_TRY(hipMemcpy(heap_used_host, h->v.heap_used, (size_t)h->v.G * 4, hipMemcpyDeviceToHost));
    SMR_HIP_TRY(hipMemcpy(full_host, h->v.full, (size_t)h->v.G, hipMemcpyDeviceToHost));
    return SMR_OK;
}

/* debug / measurement only: the one device allocation that holds the store -- what a wholesale copy of it would move -- and
 * where its nine arrays begin in it: hash, koff, klen, voff, vlen [slots][G], heap [G][heap_bytes], heap_used, full, n_keys [G] */
int smr_skv_debug_arena(smr_skv *h, void **base_dev, uint64_t *n_bytes, uint64_t offsets[9]) {
    if (!h || !base_dev || !n_bytes || !offsets) return fail(SMR_ERR_ARG, "skv: null argument");
    const SkvView &v = h->v;
    const void *const at[9] = {v.hash, v.koff, v.klen, v.voff, v.vlen, v.heap, v.heap_used, v.full, v.n_keys};
    *base_dev = h->arena.base; *n_bytes = h->arena.size;
    for (int k = 0; k < 9; k++) offsets[k] = (uint64_t)((const char *)at[k] - h->arena.base);
    return SMR_OK;
}

/* debug: host copy of bytes [off, off + len) of that allocation (synchronises) */
int smr_skv_debug_read(smr_skv *h, uint64_t off, uint64_t len, uint8_t *host_buf) {
    if (!h || (!host_buf && len)) return fail(SMR_ERR_ARG, "skv: null argument");
    if (off > h->arena.size || len > h->arena.size - off) return fail(SMR_ERR_ARG, "skv: bytes outside the store's allocation");
    SMR_HIP_TRY(hipDeviceSynchronize());
    if (len) SMR_HIP_TRY(hipMemcpy(host_buf, h->arena.base + off, len, hipMemcpyDeviceToHost));
    return SMR_OK;
}

/* ---- save / load of the store's state on the device (skv_snapshot.h: the image and its kernels) -------------------------------- */
}  // extern "C"

struct smr_skv_snapshot : SnapObj<SkvSnapHdr, 2> {               // buf: header, n_keys, full, then the records and their bytes at their capacities;
    uint32_t G = 0;                                              // cap: records, bytes; scratch: skv_snapshot.h's SkvSnapScratch
    uint32_t scratch_slots = 0;                                  // what the scratch was laid out for (with G and cap[0])
    uint64_t scratch_recs = 0, scratch_bytes = 0;
};

namespace smr {
// what is the store's own of a snapshot object and its calls (snapshot_common.h: SnapObj)
struct SkvSnap {
    static constexpr const char *WHAT = "skv snapshot: ", *GWHAT = "skv groups: ", *NOUN = "store", *LIST_OF = "";
    static constexpr bool LIST_FIRST = false;
    static uint32_t groups_of(const smr_skv *st) { return st->v.G; }
    static int init(smr_skv_snapshot *, const smr_skv *) { return SMR_OK; }
    // every entry live, the heap all live bytes, every record's run padded by up to 15
    static void need(const smr_skv_snapshot *s, const smr_skv *st, uint64_t (&n)[2]) {
        n[0] = (uint64_t)s->G * st->v.slots;
        n[1] = (uint64_t)s->G * ((st->v.heap_bytes + 15ull * st->v.slots) & ~15ull);
    }
    static void counts(const SkvSnapHdr &h, uint64_t (&n)[2]) { n[0] = h.n_records; n[1] = h.byte_bytes; }
    static uint64_t dev_bytes(const smr_skv_snapshot *s) { return skvsnap_dev_bytes(skvsnap_geom(s->G), s->cap[0]) + s->cap[1] + 16; }
    static int copy(const smr_skv_snapshot *s, uint8_t *host, const SkvSnapHdr &h, bool to_host) {
        const SkvSnapGeom q = skvsnap_geom(s->G);
        return snap_copy_sections(s->buf.dev, host, q.fixed, to_host,
                                  {{skvsnap_dev_rec(q), 16 * h.n_records, skvsnap_bytes_at(q, h.n_records) - q.fixed},
                                   {skvsnap_dev_bytes(q, s->cap[0]), h.byte_bytes, h.byte_bytes}});
    }
    static int load_fits(const smr_skv_snapshot *s, const smr_skv *st, const char *what, bool) {
        if (s->hdr.n_groups != s->G) return fail(SMR_ERR_ARG, std::string(what) + "the image is of another n_groups");
        if (s->hdr.max_keys > st->v.slots)
            return fail(SMR_ERR_ARG, std::string(what) + "a group of " + std::to_string(s->hdr.max_keys) + " keys does not fit " + std::to_string(st->v.slots) + " slots");
        if (s->hdr.max_group_bytes > st->v.heap_bytes)
            return fail(SMR_ERR_ARG, std::string(what) + "a group of " + std::to_string(s->hdr.max_group_bytes) + " bytes does not fit heap_bytes " + std::to_string(st->v.heap_bytes));
        return SMR_OK;
    }
    static int groups_pair_check(smr_skv *const *, smr_skv_snapshot *const *snaps, uint32_t, uint32_t n, SnapGroupsCall call) {
        if (call == SNAP_GROUPS_RESET) return SMR_OK;
        return snap_groups_len_check(n, snaps[0]->G, GWHAT);
    }
};

// the launches' scratch for a store of `slots` (a load: 0 -- it does not use order[], so the target's slots never make it grow):
// grows by sizes the host knows (what it held is between two launches of one call).  A snapshot serves one call at a time
static int skvsnap_scratch_room(smr_skv_snapshot *s, uint32_t slots) {
    if (s->scratch && slots <= s->scratch_slots && s->cap[0] <= s->scratch_recs) return SMR_OK;
    const uint32_t sl = slots > s->scratch_slots ? slots : s->scratch_slots;
    const uint64_t recs = s->cap[0] > s->scratch_recs ? s->cap[0] : s->scratch_recs;
    const uint64_t bytes = skvsnap_scratch_layout(s->G, sl, recs, nullptr, nullptr);
    if (s->scratch) { SMR_HIP_TRY(hipDeviceSynchronize()); (void)hipFree(s->scratch); s->scratch = nullptr; s->scratch_slots = 0; s->scratch_recs = 0; }
    hipError_t e = hipMalloc(&s->scratch, bytes);
    if (e != hipSuccess) { s->scratch = nullptr; return fail(SMR_ERR_DEVICE, std::string("skv snapshot: hipMalloc: ") + hipGetErrorString(e)); }
    s->scratch_slots = sl; s->scratch_recs = recs; s->scratch_bytes = bytes;
    return SMR_OK;
}

// the launches' arguments; s = nullptr (a reset): the geometry of n groups and no buffers
static SkvSnapArgs skvsnap_args(const smr_skv *st, const smr_skv_snapshot *s, uint32_t n = 0) {
    SkvSnapArgs A;
    memset(&A, 0, sizeof(A));
    A.v = st->v;
    if (s) {
        A.img = s->buf.dev; A.cap_rec = s->cap[0]; A.cap_bytes = s->cap[1]; A.geo = skvsnap_geom(s->G);
        (void)skvsnap_scratch_layout(s->G, s->scratch_slots, s->scratch_recs, (uint8_t *)s->scratch, &A.sc);
    } else {
        A.geo = skvsnap_geom(n);
    }
    return A;
}
static uint32_t skvsnap_wave_blocks(uint64_t items, uint32_t most) {
    const uint64_t want = (items + 3) / 4;
    return (uint32_t)(want < most ? (want ? want : 1) : most);
}

// list = nullptr: the whole store
static int skvsnap_save(smr_skv *st, smr_skv_snapshot *s, const uint32_t *list, hipStream_t stream) {
    if (int rc = skvsnap_scratch_room(s, st->v.slots)) return rc;
    const SkvSnapArgs A = skvsnap_args(st, s);
    const dim3 rank_grid(skvsnap_wave_blocks(A.geo.G, SKVSNAP_RANK_BLOCKS)), head_grid(A.geo.tiles.nblock);
    if (list) {
        hipLaunchKernelGGL(skv_snap_rank_groups, rank_grid, dim3(256), 0, stream, A, list);
        hipLaunchKernelGGL(skv_snap_head_groups<SKVSNAP_PACK>, head_grid, dim3(256), 0, stream, A, list);
    } else {
        hipLaunchKernelGGL(skv_snap_rank, rank_grid, dim3(256), 0, stream, A);
        hipLaunchKernelGGL(skv_snap_head<SKVSNAP_PACK>, head_grid, dim3(256), 0, stream, A);
    }
    hipLaunchKernelGGL(skv_snap_bytes<true>, dim3(skvsnap_wave_blocks(A.cap_rec, SKVSNAP_BYTE_BLOCKS)), dim3(256), 0, stream, A);
    SMR_HIP_TRY(hipGetLastError());
    snap_obj_saved(s);
    return SMR_OK;
}
static int skvsnap_load(smr_skv *st, smr_skv_snapshot *s, const uint32_t *list, hipStream_t stream) {
    if (int rc = skvsnap_scratch_room(s, 0)) return rc;          // (by records only: after an import into a snapshot that grew)
    SkvSnapArgs A = skvsnap_args(st, s);
    A.n_records = s->hdr.n_records;
    const dim3 head_grid(A.geo.tiles.nblock);
    hipLaunchKernelGGL(skv_snap_head<SKVSNAP_SIZES>, head_grid, dim3(256), 0, stream, A);
    if (list) hipLaunchKernelGGL(skv_snap_head_groups<SKVSNAP_UNPACK>, head_grid, dim3(256), 0, stream, A, list);
    else hipLaunchKernelGGL(skv_snap_head<SKVSNAP_UNPACK>, head_grid, dim3(256), 0, stream, A);
    if (A.n_records) hipLaunchKernelGGL(skv_snap_bytes<false>, dim3(skvsnap_wave_blocks(A.n_records, SKVSNAP_BYTE_BLOCKS)), dim3(256), 0, stream, A);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}
}  // namespace smr

extern "C" {

// worst-case room for a store like `like`, the launches' scratch included: a save into it only enqueues
static int skvsnap_made(int rc, const smr_skv *like, smr_skv_snapshot **out) {
    if (rc != SMR_OK) return rc;
    if ((rc = skvsnap_scratch_room(*out, like->v.slots)) != SMR_OK) { snap_obj_destroy(*out); *out = nullptr; }
    return rc;
}
int smr_skv_snapshot_create(const smr_skv *like, smr_skv_snapshot **out) { return skvsnap_made(snap_obj_create<SkvSnap>(like, out), like, out); }
int smr_skv_snapshot_create_groups(const smr_skv *like, uint32_t n, smr_skv_snapshot **out) {
    return skvsnap_made(snap_obj_create_groups<SkvSnap>(like, n, out), like, out);
}
void smr_skv_snapshot_destroy(smr_skv_snapshot *s) { snap_obj_destroy(s); }

int smr_skv_save_state(smr_skv *st, smr_skv_snapshot *s, void *stream) {
    if (!st || !s) return fail(SMR_ERR_ARG, "skv snapshot: null argument");
    if (s->G != st->v.G) return fail(SMR_ERR_ARG, "skv snapshot: made for another n_groups");
    if (int rc = snap_obj_room_for<SkvSnap>(s, st)) return rc;
    return skvsnap_save(st, s, nullptr, (hipStream_t)stream);
}

int smr_skv_load_state(smr_skv *st, const smr_skv_snapshot *cs, void *stream) {
    if (!st || !cs) return fail(SMR_ERR_ARG, "skv snapshot: null argument");
    smr_skv_snapshot *s = const_cast<smr_skv_snapshot *>(cs);    // (the header is read back and cached on first use)
    if (s->G != st->v.G) return fail(SMR_ERR_ARG, "skv snapshot: made for another n_groups");
    if (int rc = snap_obj_load_ready<SkvSnap>(s, st, SkvSnap::WHAT, false)) return rc;
    return skvsnap_load(st, s, nullptr, (hipStream_t)stream);
}

// ---- chosen groups between stores (the same image, the same bodies, through a group list) --------------------------------------
int smr_skv_save_groups(smr_skv *st, const uint32_t *groups_host, uint32_t n, smr_skv_snapshot *s, void *stream) {
    if (int rc = snap_groups_setup<SkvSnap>(1, &st, &s, groups_host, n, SNAP_GROUPS_SAVE)) return rc;
    if (int rc = snap_glist_upload(s->glist, groups_host, n, (hipStream_t)stream, SkvSnap::GWHAT)) return rc;
    return skvsnap_save(st, s, s->glist.dev, (hipStream_t)stream);
}

int smr_skv_load_groups(smr_skv *st, const smr_skv_snapshot *cs, const uint32_t *groups_host, uint32_t n, void *stream) {
    smr_skv_snapshot *s = const_cast<smr_skv_snapshot *>(cs);
    if (int rc = snap_groups_setup<SkvSnap>(1, &st, &s, groups_host, n, SNAP_GROUPS_LOAD)) return rc;
    if (int rc = snap_glist_upload(s->glist, groups_host, n, (hipStream_t)stream, SkvSnap::GWHAT)) return rc;
    return skvsnap_load(st, s, s->glist.dev, (hipStream_t)stream);
}

int smr_skv_reset_groups(smr_skv *st, const uint32_t *groups_host, uint32_t n, void *stream) {
    if (int rc = snap_groups_setup<SkvSnap>(1, &st, (smr_skv_snapshot *const *)nullptr, groups_host, n, SNAP_GROUPS_RESET)) return rc;
    if (int rc = snap_glist_upload(st->glist, groups_host, n, (hipStream_t)stream, SkvSnap::GWHAT)) return rc;
    const SkvSnapArgs A = skvsnap_args(st, nullptr, n);
    const uint32_t *list = st->glist.dev;
    hipLaunchKernelGGL(skv_snap_head_groups<SKVSNAP_FRESH>, dim3(A.geo.tiles.nblock), dim3(256), 0, (hipStream_t)stream, A, list);   // heap bytes are not touched
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_skv_snapshot_info_get(const smr_skv_snapshot *cs, smr_skv_snapshot_info *out) {
    if (int rc = snap_obj_info<SkvSnap>(cs, out)) return rc;
    const SkvSnapHdr &h = cs->hdr;
    out->bytes = h.bytes; out->n_records = h.n_records; out->byte_bytes = h.byte_bytes;
    out->n_groups = h.n_groups; out->max_keys = h.max_keys; out->max_group_bytes = h.max_group_bytes;
    return SMR_OK;
}

int64_t smr_skv_snapshot_export(const smr_skv_snapshot *cs, uint8_t *host, uint64_t cap) { return snap_obj_export<SkvSnap>(cs, host, cap); }

int smr_skv_snapshot_import(smr_skv_snapshot *s, const uint8_t *host, uint64_t len) {
    if (!s || !host) return fail(SMR_ERR_ARG, "skv snapshot: null argument");
    SkvSnapHdr h;
    if (int rc = snap_import_prologue(host, len, SKVSNAP_MAGIC, SKVSNAP_VERSION, SkvSnap::WHAT, h, "string store")) return rc;
    if (h.n_groups != s->G || h.reserved0 || h.reserved[0] || h.reserved[1]) return fail(SMR_ERR_ARG, "skv snapshot: the image is of another n_groups");
    const SkvSnapGeom q = skvsnap_geom(s->G);
    const uint64_t G = s->G;
    if (snap_truncated(len, q.fixed, h.bytes) || h.n_records > (h.bytes - q.fixed) / 16 || h.bytes - skvsnap_bytes_at(q, h.n_records) != h.byte_bytes ||
        skvsnap_bytes_at(q, h.n_records) > h.bytes || (h.byte_bytes & 15))
        return fail(SMR_ERR_ARG, "skv snapshot: truncated image, or its sizes do not add up");
    const auto bad = [](const char *what) { return fail(SMR_ERR_ARG, std::string("skv snapshot: malformed image: ") + what); };
    const auto u32at = [&](uint64_t off, uint64_t i) { uint32_t x; memcpy(&x, host + off + 4 * i, 4); return x; };
    const uint64_t o_rec = q.fixed, o_bytes = skvsnap_bytes_at(q, h.n_records);
    if (!snap_pad_is_zero(host, q.o_nkeys, 4 * G) || !snap_pad_is_zero(host, q.o_full, G)) return bad("padding is not zero");
    for (uint64_t b = o_rec + 16 * h.n_records; b < o_bytes; b++) if (host[b]) return bad("padding is not zero");
    uint64_t total = 0;
    uint32_t max_keys = 0;
    for (uint64_t x = 0; x < G; x++) {
        const uint32_t c = u32at(q.o_nkeys, x);
        total += c; max_keys = c > max_keys ? c : max_keys;
        if (host[q.o_full + x] > 1) return bad("a full flag that is neither 0 nor 1");
    }
    if (total != h.n_records || max_keys != h.max_keys) return bad("the groups' n_keys contradict the header's counts");
    // the records against the counts, in the image's order: tile, rank, position; per group strictly ascending (hash, klen, key)
    uint64_t pos = 0, off = 0, max_bytes = 0;
    for (uint64_t t0 = 0; t0 < G; t0 += 64) {
        const uint32_t lanes = (uint32_t)(G - t0 < 64 ? G - t0 : 64);
        uint32_t c[64], rows = 0;
        uint64_t prev_h[64], prev_at[64], raw[64];
        uint32_t prev_kl[64];
        for (uint32_t l = 0; l < lanes; l++) { c[l] = u32at(q.o_nkeys, t0 + l); rows = c[l] > rows ? c[l] : rows; raw[l] = 0; }
        for (uint32_t k = 0; k < rows; k++)
            for (uint32_t l = 0; l < lanes; l++) {
                if (k >= c[l]) continue;
                SkvSnapRec r;
                memcpy(&r, host + o_rec + 16 * pos, 16);
                pos++;
                if (r.klen == SKV_EMPTY) return bad("a key length that marks a free entry");
                const uint64_t rl = (uint64_t)r.klen + r.vlen, rl16 = snap_a16(rl);
                if (rl16 > h.byte_bytes - off) return bad("the records ask for more bytes than the image holds");
                const uint8_t *const kp = host + o_bytes + off;
                if (skvsnap_fnv1a(kp, r.klen) != r.hash) return bad("a record's hash is not its key's");
                for (uint64_t b = rl; b < rl16; b++) if (kp[b]) return bad("padding is not zero");
                if (k) {
                    const uint8_t *const pp = host + o_bytes + prev_at[l];
                    int cmp = prev_h[l] < r.hash ? -1 : (prev_h[l] > r.hash ? 1 : (prev_kl[l] < r.klen ? -1 : (prev_kl[l] > r.klen ? 1 : memcmp(pp, kp, r.klen))));
                    if (cmp >= 0) return bad("a group's records are not in strictly ascending rank order");
                }
                prev_h[l] = r.hash; prev_kl[l] = r.klen; prev_at[l] = off;
                off += rl16; raw[l] += rl;
            }
        for (uint32_t l = 0; l < lanes; l++) max_bytes = raw[l] > max_bytes ? raw[l] : max_bytes;
    }
    if (off != h.byte_bytes || max_bytes != h.max_group_bytes) return bad("the header's counts contradict the records");
    return snap_obj_import_bytes<SkvSnap>(s, host, h);
}

/* debug / measurement only: the snapshot's device buffer (the image at its capacities) */
int smr_skv_snapshot_debug_buffer(const smr_skv_snapshot *s, void **dev, uint64_t *n_bytes) {
    if (!s || !dev || !n_bytes) return fail(SMR_ERR_ARG, "skv snapshot: null argument");
    *dev = s->buf.dev; *n_bytes = SkvSnap::dev_bytes(s);
    return SMR_OK;
}

}  // extern "C"
