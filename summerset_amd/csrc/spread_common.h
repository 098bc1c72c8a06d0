// What the library's two spread objects (ep_spread.hip, rsp_spread.hip) have in common -- host code only: where a replica lives,
// the seating of a rank's replicas, how a message list becomes an exchange's buffers and split sizes, the arena, and the bodies of
// the small entry points.  The message lists, the slots' fields and the kernels stay with the engines.
//
// The layout rule, the same as summerset_amd/spread_plan.py `build` (tests/golden/spread_plan_digests.json and the split-size
// check of tests/test_spread_plan_digests.py pin the two to each other): every rank derives an exchange's message list in one
// canonical order; a rank's send buffer holds the messages it is the source of, stable-sorted by destination rank, at running
// offsets, its receive buffer the ones it is the destination of, stable-sorted by source rank.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "smr_common.h"

namespace smr {

// replica r of block b lives on rank (b + r) mod world
static inline uint32_t spread_home(uint32_t b, uint32_t r, uint32_t world) { return (b + r) % world; }

struct SpreadPlan {                                 // one exchange, as this rank sees it
    std::vector<uint64_t> in_split, out_split;      // bytes to / from every rank
    uint64_t n_send = 0, n_recv = 0;
    uint8_t *sbuf = nullptr, *rbuf = nullptr;
};
struct SpreadJob {                                  // what a spread object knows of the job and of its open tick
    uint32_t world = 0, rank = 0, R = 0;
    std::vector<uint32_t> block_groups;
    std::vector<int> rep_of;                        // [b * R + r] -> index of the replica in create's order, -1
    char *arena = nullptr;
    smr_comm *comm = nullptr;
    uint32_t next_seg = 0;
    uint64_t bytes_sent = 0;
};

// ---- create: the arguments, then the rank's replicas into rep_of --------------------------------------------------------------
static inline int spread_check_args(const std::string &who, const void *out, const void *reps, const uint32_t *rep_block, const uint8_t *rep_id, uint32_t n_reps,
                                    const uint32_t *block_groups, uint32_t world, uint32_t rank, uint8_t population) {
    if (!out || !block_groups || (n_reps && (!reps || !rep_block || !rep_id))) return fail(SMR_ERR_ARG, who + ": null argument");
    if (world == 0 || rank >= world) return fail(SMR_ERR_ARG, who + ": rank / world");
    if (population < 3 || population > SMR_MAX_REPLICAS) return fail(SMR_ERR_ARG, who + ": population must be in 3..8");
    return SMR_OK;
}
// replica i is (rep_block[i], rep_id[i]): every one at its home, once, and every replica whose home this rank is
template <class E>
static inline int spread_seat(SpreadJob *s, const std::string &who, E *const *reps, const uint32_t *rep_block, const uint8_t *rep_id, uint32_t n_reps,
                              const uint32_t *block_groups, uint32_t world, uint32_t rank, uint8_t population) {
    s->world = world; s->rank = rank; s->R = population;
    s->block_groups.assign(block_groups, block_groups + world);
    s->rep_of.assign((size_t)world * population, -1);
    const uint64_t R = population;
    for (uint32_t i = 0; i < n_reps; i++) {
        const uint32_t b = rep_block[i], r = rep_id[i];
        if (!reps[i] || b >= world || r >= population || spread_home(b, r, world) != rank || !block_groups[b] || s->rep_of[(size_t)b * R + r] >= 0)
            return fail(SMR_ERR_ARG, who + ": replica r of block b lives on rank (b + r) mod world, once, and only where the block has groups");
        s->rep_of[(size_t)b * R + r] = (int)i;
    }
    for (uint32_t b = 0; b < world; b++)
        for (uint32_t r = 0; r < population; r++)
            if (block_groups[b] && spread_home(b, r, world) == rank && s->rep_of[(size_t)b * R + r] < 0)
                return fail(SMR_ERR_ARG, who + ": a replica that lives on this rank was not handed over");
    return SMR_OK;
}

// ---- the plan layout ---------------------------------------------------------------------------------------------------------------
// a message that goes through the exchange; slot: the engine's index for it.  spread_layout fills soff where src is this rank and
// roff where dst is (a message from this rank to itself has both: it goes through the rank's own segment)
struct SpreadMsg { uint32_t src, dst; size_t slot; uint64_t bytes, soff, roff; };
static inline void spread_layout(std::vector<SpreadMsg> &msgs, uint32_t rank, uint32_t world, SpreadPlan &p) {
    p.in_split.assign(world, 0); p.out_split.assign(world, 0);
    std::vector<SpreadMsg *> send, recv;
    for (SpreadMsg &m : msgs) {
        if (m.src == rank) send.push_back(&m);
        if (m.dst == rank) recv.push_back(&m);
    }
    std::stable_sort(send.begin(), send.end(), [](const SpreadMsg *x, const SpreadMsg *y) { return x->dst < y->dst; });
    std::stable_sort(recv.begin(), recv.end(), [](const SpreadMsg *x, const SpreadMsg *y) { return x->src < y->src; });
    for (SpreadMsg *m : send) { m->soff = p.n_send; p.n_send += m->bytes; p.in_split[m->dst] += m->bytes; }
    for (SpreadMsg *m : recv) { m->roff = p.n_recv; p.n_recv += m->bytes; p.out_split[m->src] += m->bytes; }
}

// ---- the arena: sizes first, one allocation, then the pointers ----------------------------------------------------------------------
struct SpreadArena {
    size_t bytes = 0;
    size_t take(size_t n) { size_t o = bytes; bytes = (bytes + n + 255) & ~(size_t)255; return o; }
    // one allocation of everything taken (+ 256), cleared: *out stays null where the allocation failed, the result is the clear's
    hipError_t alloc_zeroed(char **out) const {
        if (hipMalloc((void **)out, bytes + 256) != hipSuccess) { *out = nullptr; return hipErrorOutOfMemory; }
        return hipMemset(*out, 0, bytes + 256);
    }
};

// ---- the bodies of smr_*_spread_buffers / _bind_comm / _abort_tick, and a segment's place in the open tick ---------------------------
static inline int spread_buffers(const SpreadJob *s, const std::string &who, const SpreadPlan *p, void **send_dev, uint64_t *send_bytes, void **recv_dev,
                                 uint64_t *recv_bytes) {
    if (!s || !p || !send_dev || !send_bytes || !recv_dev || !recv_bytes) return fail(SMR_ERR_ARG, who + ": bad argument");
    *send_dev = p->sbuf; *recv_dev = p->rbuf;
    for (uint32_t k = 0; k < s->world; k++) { send_bytes[k] = p->in_split[k]; recv_bytes[k] = p->out_split[k]; }
    return SMR_OK;
}
static inline int spread_bind_comm(SpreadJob *s, const std::string &who, smr_comm *comm) {
    if (!s) return fail(SMR_ERR_ARG, who + ": null argument");
    if (comm) {
        uint64_t info[5];
        int rc = smr_comm_info(comm, info);
        if (rc != SMR_OK) return rc;
        if (info[0] != s->rank || info[1] != s->world) return fail(SMR_ERR_ARG, who + ": the communicator's rank / world are not the job's");
    }
    s->comm = comm;
    return SMR_OK;
}
static inline int spread_abort_tick(SpreadJob *s, const std::string &who) {
    if (!s) return fail(SMR_ERR_ARG, who + ": null argument");
    s->next_seg = 0;
    return SMR_OK;
}
static inline int spread_in_order(const SpreadJob *s, const std::string &who, uint32_t seg) {
    if (seg != s->next_seg) return fail(SMR_ERR_STATE, who + ": segment " + std::to_string(seg) + " out of order (the open tick expects " + std::to_string(s->next_seg) + ")");
    return SMR_OK;
}

}  // namespace smr
