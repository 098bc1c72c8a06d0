// Device-resident KV state machine over G groups: StateMachineExecutorTask::execute
// (src/server/statemach.rs:193-202) applied to each group's commands in submission order, lane = group.
// Model shared with qread.hip and the EPaxos execution kernel: keys < K, a value is a 32-bit token, 0 = None.
// The table kv[K][G] is what a stable leased leader answers ReadQueries from (smr_qread_handle_read_query).
#include <string.h>

#include "smr_common.h"

namespace smr {

struct KvView { uint32_t G, K; uint32_t *kv; };

// kind[B][G]: 0 Get, 1 Put, anything else = no command in that row; res = Get: value, Put: old_value (0 = None)
__global__ __launch_bounds__(256) void kv_execute_kernel(const KvView v, uint32_t B, const uint8_t *__restrict__ kind,
                                                         const uint8_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                         uint32_t *__restrict__ res) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= v.G) return;
    for (uint32_t i = 0; i < B; i++) {
        const size_t o = (size_t)i * v.G + g;
        const uint32_t kd = kind[o], k = key[o];
        uint32_t r = 0;
        if (kd <= 1 && k < v.K) {
            uint32_t *cell = &v.kv[(size_t)k * v.G + g];
            r = *cell;                                       // Get: state.get(key).cloned(); Put: what insert() returns
            if (kd == 1) *cell = val[o];                     // state.insert(key, value)
        }
        res[o] = r;
    }
}

}  // namespace smr

#include "kv_snapshot.h"

using namespace smr;

struct smr_kv {
    KvView v;
    SnapGroupListBuf glist;   // smr_kv_reset_groups' list on the device
};

extern "C" {

int smr_kv_create(uint32_t n_groups, uint32_t n_keys, smr_kv **out) {
    if (!out || !n_groups || !n_keys || n_keys > 255) return fail(SMR_ERR_ARG, "kv: n_groups > 0 and n_keys in 1..255");
    smr_kv *h = new smr_kv();
    h->v.G = n_groups; h->v.K = n_keys; h->v.kv = nullptr;
    const size_t bytes = (size_t)n_keys * n_groups * 4;
    hipError_t e = hipMalloc((void **)&h->v.kv, bytes);
    static_assert(KV_INIT_TOKEN == 0, "create fills bytes");     // a cell's initial value is kv_snapshot.h's (shared with smr_kv_reset_groups)
    if (e == hipSuccess) e = hipMemset(h->v.kv, (int)KV_INIT_TOKEN, bytes);
    if (e != hipSuccess) {
        if (h->v.kv) (void)hipFree(h->v.kv);
        delete h;
        return fail(SMR_ERR_DEVICE, std::string("kv: alloc: ") + hipGetErrorString(e));
    }
    *out = h;
    return SMR_OK;
}

void smr_kv_destroy(smr_kv *h) {
    if (!h) return;
    snap_glist_free(h->glist);
    if (h->v.kv) (void)hipFree(h->v.kv);
    delete h;
}

int smr_kv_execute(smr_kv *h, uint32_t n_rows, const uint8_t *kind_dev, const uint8_t *key_dev, const uint32_t *val_dev,
                   uint32_t *res_dev, void *stream) {
    if (!h || !kind_dev || !key_dev || !val_dev || !res_dev) return fail(SMR_ERR_ARG, "kv: null argument");
    if (!n_rows) return SMR_OK;
    hipLaunchKernelGGL(kv_execute_kernel, dim3((h->v.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->v, n_rows, kind_dev, key_dev,
                       val_dev, res_dev);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_kv_table(smr_kv *h, uint32_t **kv_dev) {
    if (!h || !kv_dev) return fail(SMR_ERR_ARG, "kv: null argument");
    *kv_dev = h->v.kv;
    return SMR_OK;
}

int smr_kv_dump(smr_kv *h, uint32_t *kv_host) {
    if (!h || !kv_host) return fail(SMR_ERR_ARG, "kv: null argument");
    SMR_HIP_TRY(hipDeviceSynchronize());
    SMR_HIP_TRY(hipMemcpy(kv_host, h->v.kv, (size_t)h->v.K * h->v.G * 4, hipMemcpyDeviceToHost));
    return SMR_OK;
}

/* ---- save / load of the table on the device (kv_snapshot.h: the image and its kernel) ---------------------------------------- */
}  // extern "C"

struct smr_kv_snapshot : SnapObj<KvSnapHdr, 1> {                 // buf: the image, dense; cap: cells
    uint32_t G = 0, K = 0;
};

namespace smr {
struct KvSnap {
    static constexpr const char *WHAT = "kv snapshot: ", *GWHAT = "kv groups: ", *NOUN = "table", *LIST_OF = "";
    static constexpr bool LIST_FIRST = false;
    static uint32_t groups_of(const smr_kv *t) { return t->v.G; }
    static int init(smr_kv_snapshot *s, const smr_kv *like) { s->K = like->v.K; return SMR_OK; }
    static void need(const smr_kv_snapshot *s, const smr_kv *, uint64_t (&n)[1]) { n[0] = kvsnap_cells(s->G, s->K); }
    static void counts(const KvSnapHdr &h, uint64_t (&n)[1]) { n[0] = kvsnap_cells(h.n_groups, h.n_keys); }
    static uint64_t dev_bytes(const smr_kv_snapshot *s) { return sizeof(KvSnapHdr) + snap_a8(4 * s->cap[0]) + 16; }
    static int copy(const smr_kv_snapshot *s, uint8_t *host, const KvSnapHdr &h, bool to_host) {   // (the image is dense)
        SMR_HIP_TRY(to_host ? hipMemcpy(host, s->buf.dev, h.bytes, hipMemcpyDeviceToHost) : hipMemcpy(s->buf.dev, host, h.bytes, hipMemcpyHostToDevice));
        return SMR_OK;
    }
    static int load_fits(const smr_kv_snapshot *s, const smr_kv *t, const char *what, bool) {
        if (s->hdr.n_groups != s->G || s->hdr.n_keys != s->K) return fail(SMR_ERR_ARG, std::string(what) + "the image is of another n_groups / n_keys");
        if (s->hdr.n_keys != t->v.K)
            return fail(SMR_ERR_ARG, std::string(what) + "an image of " + std::to_string(s->hdr.n_keys) + " keys and a table of " + std::to_string(t->v.K));
        return SMR_OK;
    }
    static int groups_pair_check(smr_kv *const *ts, smr_kv_snapshot *const *snaps, uint32_t, uint32_t n, SnapGroupsCall call) {
        if (call == SNAP_GROUPS_RESET) return SMR_OK;
        if (snaps[0]->K != ts[0]->v.K) return fail(SMR_ERR_ARG, "kv groups: the snapshot was made for another n_keys");
        return snap_groups_len_check(n, snaps[0]->G, GWHAT);
    }
};
static KvSnapArgs kvsnap_args(const smr_kv *t, const smr_kv_snapshot *s, uint32_t n) {
    KvSnapArgs A;
    memset(&A, 0, sizeof(A));
    A.v = t->v; A.n = n;
    if (s) { A.img = s->buf.dev; A.cap_cells = s->cap[0]; }
    return A;
}
static dim3 kvsnap_grid(const KvSnapArgs &A) {
    const uint64_t want = (kvsnap_cells(A.n, A.v.K) + 255) / 256;
    return dim3((uint32_t)(want < KVSNAP_BLOCKS ? (want ? want : 1) : KVSNAP_BLOCKS));
}
static bool kvsnap_like(const smr_kv_snapshot *s, const smr_kv *t) { return s->G == t->v.G && s->K == t->v.K; }
}  // namespace smr

extern "C" {

int smr_kv_snapshot_create(const smr_kv *like, smr_kv_snapshot **out) { return snap_obj_create<KvSnap>(like, out); }
int smr_kv_snapshot_create_groups(const smr_kv *like, uint32_t n, smr_kv_snapshot **out) { return snap_obj_create_groups<KvSnap>(like, n, out); }
void smr_kv_snapshot_destroy(smr_kv_snapshot *s) { snap_obj_destroy(s); }

int smr_kv_save_state(smr_kv *t, smr_kv_snapshot *s, void *stream) {
    if (!t || !s) return fail(SMR_ERR_ARG, "kv snapshot: null argument");
    if (!kvsnap_like(s, t)) return fail(SMR_ERR_ARG, "kv snapshot: made for another n_groups / n_keys");
    if (int rc = snap_obj_room_for<KvSnap>(s, t)) return rc;
    const KvSnapArgs A = kvsnap_args(t, s, s->G);
    hipLaunchKernelGGL(kv_snap<KVSNAP_PACK>, kvsnap_grid(A), dim3(256), 0, (hipStream_t)stream, A);
    SMR_HIP_TRY(hipGetLastError());
    snap_obj_saved(s);
    return SMR_OK;
}

int smr_kv_load_state(smr_kv *t, const smr_kv_snapshot *cs, void *stream) {
    if (!t || !cs) return fail(SMR_ERR_ARG, "kv snapshot: null argument");
    smr_kv_snapshot *s = const_cast<smr_kv_snapshot *>(cs);      // (the header is read back and cached on first use)
    if (!kvsnap_like(s, t)) return fail(SMR_ERR_ARG, "kv snapshot: made for another n_groups / n_keys");
    if (int rc = snap_obj_load_ready<KvSnap>(s, t, KvSnap::WHAT, false)) return rc;
    const KvSnapArgs A = kvsnap_args(t, s, s->G);
    hipLaunchKernelGGL(kv_snap<KVSNAP_UNPACK>, kvsnap_grid(A), dim3(256), 0, (hipStream_t)stream, A);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_kv_save_groups(smr_kv *t, const uint32_t *groups_host, uint32_t n, smr_kv_snapshot *s, void *stream) {
    if (int rc = snap_groups_setup<KvSnap>(1, &t, &s, groups_host, n, SNAP_GROUPS_SAVE)) return rc;
    if (int rc = snap_glist_upload(s->glist, groups_host, n, (hipStream_t)stream, KvSnap::GWHAT)) return rc;
    const KvSnapArgs A = kvsnap_args(t, s, n);
    const uint32_t *list = s->glist.dev;
    hipLaunchKernelGGL(kv_snap_groups<KVSNAP_PACK>, kvsnap_grid(A), dim3(256), 0, (hipStream_t)stream, A, list);
    SMR_HIP_TRY(hipGetLastError());
    snap_obj_saved(s);
    return SMR_OK;
}

int smr_kv_load_groups(smr_kv *t, const smr_kv_snapshot *cs, const uint32_t *groups_host, uint32_t n, void *stream) {
    smr_kv_snapshot *s = const_cast<smr_kv_snapshot *>(cs);
    if (int rc = snap_groups_setup<KvSnap>(1, &t, &s, groups_host, n, SNAP_GROUPS_LOAD)) return rc;
    if (int rc = snap_glist_upload(s->glist, groups_host, n, (hipStream_t)stream, KvSnap::GWHAT)) return rc;
    const KvSnapArgs A = kvsnap_args(t, s, n);
    const uint32_t *list = s->glist.dev;
    hipLaunchKernelGGL(kv_snap_groups<KVSNAP_UNPACK>, kvsnap_grid(A), dim3(256), 0, (hipStream_t)stream, A, list);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_kv_reset_groups(smr_kv *t, const uint32_t *groups_host, uint32_t n, void *stream) {
    if (int rc = snap_groups_setup<KvSnap>(1, &t, (smr_kv_snapshot *const *)nullptr, groups_host, n, SNAP_GROUPS_RESET)) return rc;
    if (int rc = snap_glist_upload(t->glist, groups_host, n, (hipStream_t)stream, KvSnap::GWHAT)) return rc;
    const KvSnapArgs A = kvsnap_args(t, nullptr, n);
    const uint32_t *list = t->glist.dev;
    hipLaunchKernelGGL(kv_snap_groups<KVSNAP_FRESH>, kvsnap_grid(A), dim3(256), 0, (hipStream_t)stream, A, list);
    SMR_HIP_TRY(hipGetLastError());
    return SMR_OK;
}

int smr_kv_snapshot_info_get(const smr_kv_snapshot *cs, smr_kv_snapshot_info *out) {
    if (int rc = snap_obj_info<KvSnap>(cs, out)) return rc;
    out->bytes = cs->hdr.bytes; out->n_groups = cs->hdr.n_groups; out->n_keys = cs->hdr.n_keys;
    return SMR_OK;
}

int64_t smr_kv_snapshot_export(const smr_kv_snapshot *cs, uint8_t *host, uint64_t cap) { return snap_obj_export<KvSnap>(cs, host, cap); }

int smr_kv_snapshot_import(smr_kv_snapshot *s, const uint8_t *host, uint64_t len) {
    if (!s || !host) return fail(SMR_ERR_ARG, "kv snapshot: null argument");
    KvSnapHdr h;
    if (int rc = snap_import_prologue(host, len, KVSNAP_MAGIC, KVSNAP_VERSION, KvSnap::WHAT, h, "token table")) return rc;
    if (h.n_groups != s->G || h.n_keys != s->K) return fail(SMR_ERR_ARG, "kv snapshot: the image is of another n_groups / n_keys");
    for (int j = 0; j < 5; j++) if (h.reserved[j]) return fail(SMR_ERR_ARG, "kv snapshot: malformed image: reserved words are not zero");
    if (h.bytes != kvsnap_bytes(s->G, s->K) || h.bytes > len) return fail(SMR_ERR_ARG, "kv snapshot: truncated image, or its sizes do not add up");
    if (!snap_pad_is_zero(host, sizeof(KvSnapHdr), 4 * kvsnap_cells(s->G, s->K))) return fail(SMR_ERR_ARG, "kv snapshot: malformed image: padding is not zero");
    return snap_obj_import_bytes<KvSnap>(s, host, h);
}

}  // extern "C"
