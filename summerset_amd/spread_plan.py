"""Layout L2, the part that is the same for every engine: where a replica lives, how a list of messages
becomes one exchange's buffers and split sizes, and the exchange itself.  spread_mp / spread_ep / spread_rsp build their message
lists (that is the protocol) and hand them here; csrc/spread_common.h is the same rule in the library, and
tests/golden/spread_plan_digests.json pins the two to each other.

The rule: every rank derives the exchange's message list in ONE canonical order (blocks ascending, then what the engine says).
A rank's send buffer holds the messages it is the source of, stable-sorted by destination rank, at running offsets; its receive
buffer the messages it is the destination of, stable-sorted by source rank.  So the segment rank s sends to d and the segment d
receives from s hold the same messages in the same order, and `in_split[d]` at s equals `out_split[s]` at d."""
import ctypes as C


def home(block, replica, world):
    """the rank replica `replica` of block `block` lives on"""
    return (block + replica) % world


def build(torch, msgs, size, rank, world, device, min_bytes):
    """msgs: the exchange's messages (src rank, dst rank, key) in canonical order, the same list on every rank; size(key): a
    message's bytes; min_bytes: the buffers are never empty tensors.  soff / roff: key -> offset in sbuf / rbuf, in buffer order."""
    send = sorted([m for m in msgs if m[0] == rank], key=lambda m: m[1])            # stable: canonical order per destination
    recv = sorted([m for m in msgs if m[1] == rank], key=lambda m: m[0])
    in_split, out_split, soff, roff = [0] * world, [0] * world, {}, {}
    n_send = n_recv = 0
    for _, dst, key in send:
        soff[key], n = n_send, size(key)
        n_send += n
        in_split[dst] += n
    for src, _, key in recv:
        roff[key], n = n_recv, size(key)
        n_recv += n
        out_split[src] += n
    return dict(soff=soff, roff=roff, in_split=in_split, out_split=out_split, n_send=n_send, n_recv=n_recv,
                sbuf=torch.zeros(max(n_send, min_bytes), dtype=torch.uint8, device=device),
                rbuf=torch.zeros(max(n_recv, min_bytes), dtype=torch.uint8, device=device))


def exchange(plan, world, comm=None):
    """ONE all-to-all on the plan's buffers: the library's (comm: smr_comm_exchange, RCCL send / recv pairs) or
    torch.distributed's on exactly the planned bytes; a job of one rank copies what it sends to itself"""
    if world > 1 and comm is not None:
        comm.exchange(plan["sbuf"], plan["in_split"], plan["rbuf"], plan["out_split"])
    elif world > 1:
        import torch.distributed as dist
        dist.all_to_all_single(plan["rbuf"][:plan["n_recv"]], plan["sbuf"][:plan["n_send"]], output_split_sizes=plan["out_split"],
                               input_split_sizes=plan["in_split"])
    elif plan["n_send"]:
        plan["rbuf"][:plan["n_recv"]].copy_(plan["sbuf"][:plan["n_send"]])


def segment_pairs(plans):
    """(destination views, source views) of the all-to-all of a job whose ranks all live in this process: plans[r] = rank r's plan
    of the exchange; rank s's segment for d -> d's segment from s, the empty segments left out"""
    dsts, srcs = [], []
    for s, p in enumerate(plans):
        so = 0
        for d, n in enumerate(p["in_split"]):
            q = plans[d]
            ro = sum(q["out_split"][:s])
            assert q["out_split"][s] == n
            if n:
                dsts.append(q["rbuf"][ro:ro + n])
                srcs.append(p["sbuf"][so:so + n])
            so += n
    return dsts, srcs


def copy_between(plans):
    """that all-to-all as one `copy_` per segment pair: what the EPaxos and RSPaxos jobs do, whose segments are few and large (the
    shards).  One multi-tensor copy, which is how spread_mp moves its many images, moves a byte per lane: on the device it took the
    RSPaxos tick from 0.85 to 1.08 ms (profiles/spread_refactor_ab.log)."""
    for dst, src in zip(*segment_pairs(plans)):
        dst.copy_(src)


def check_comm(comm, rank, world):
    """`comm` (summerset_amd.comm.Comm, or None) is this rank's end of the job's communicator"""
    if comm is not None and (comm.world != world or comm.rank != rank):
        raise ValueError("the communicator is rank %d of %d, the job's rank is %d of %d" % (comm.rank, comm.world, rank, world))


def replica_arrays(reps, groups, world):
    """what smr_*_spread_create takes for a rank's replicas: (order, handles, blocks, ids, n, groups per block) with the
    replicas (block, replica) -> engine in sorted order; groups[b] = block b's (lo, hi)"""
    order = sorted(reps)
    n = len(order)
    return (order, (C.c_void_p * max(n, 1))(*[reps[k]._h for k in order]), (C.c_uint32 * max(n, 1))(*[k[0] for k in order]),
            (C.c_uint8 * max(n, 1))(*[k[1] for k in order]), n, (C.c_uint32 * world)(*[groups[b][1] - groups[b][0] for b in range(world)]))


def library_buffers(buffers_fn, h, k, world):
    """exchange k of a library spread object (smr_*_spread_buffers): (send pointer, receive pointer, in_split, out_split)"""
    from . import _lib
    sp, rp = C.c_void_p(), C.c_void_p()
    sb, rb = (C.c_uint64 * world)(), (C.c_uint64 * world)()
    _lib.check(buffers_fn(h, k, C.byref(sp), sb, C.byref(rp), rb))
    return sp.value, rp.value, [int(x) for x in sb], [int(x) for x in rb]


def tensor_over(torch, ptr, nbytes, device):
    """a uint8 tensor over `nbytes` of device (or, on the emulator, host) memory the library owns"""
    import numpy as np
    if str(device).startswith("cuda"):
        class _Mem:                                          # __cuda_array_interface__: torch.as_tensor wraps device memory without a copy
            pass
        m = _Mem()
        m.__cuda_array_interface__ = dict(shape=(int(nbytes),), typestr="|u1", data=(int(ptr), False), version=2)
        return torch.as_tensor(m, device=device)
    return torch.from_numpy(np.ctypeslib.as_array((C.c_uint8 * int(nbytes)).from_address(int(ptr))))
