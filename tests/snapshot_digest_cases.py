"""One exported image of every snapshot kind from a fixed-seed schedule, against the SHA-256 recorded in
tests/golden/snapshot_image_digests.json: the bytes of the images do not move.  The bodies of tests/test_snapshot_digests.py
(emulator, dev = "cpu") and tests/test_zzzz_snapshot_digests_gpu.py (device).

The schedules are the existing case bodies' (tests/*_snapshot_cases.py), driven with explicit seeds at the smallest shape that has
more than one tile and a partly filled last one -- 130 groups, window 8, five replicas; 70 groups for the stores -- so the checks
those bodies make against the oracle run here too (`rsp_store` says what it leaves out).  The image is what the snapshot class's `export` handed to the body: `export`
is watched while the body runs, nothing of the product is replaced.  tools/make_snapshot_digests.py writes the file."""
import contextlib
import hashlib
import json
import os
import struct
from unittest import mock

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snapshot_image_digests.json")


@contextlib.contextmanager
def exports_of(cls, on_info=False):
    """every image `cls.export` returns inside the block, in order.  on_info: a body that never exports (it only asks `info()`)
    -- every `info()` from outside is followed by an export"""
    out, orig, orig_info, busy = [], cls.export, cls.info, []

    def export(self):
        busy.append(1)
        try:
            img = orig(self)
        finally:
            busy.pop()
        out.append(img)
        return img

    def info(self):
        d = orig_info(self)
        if on_info and not busy:
            export(self)
        return d
    with mock.patch.object(cls, "export", export), mock.patch.object(cls, "info", info):
        yield out


def _last(imgs, pred, what):
    pick = [x for x in imgs if pred(x)]
    assert pick, ("no exported image has", what, len(imgs))
    return pick[-1]


def _u64(img, off):
    return struct.unpack_from("<Q", img, off)[0]


def mp_cluster(dev, oracle, G=130, R=5, W=8):
    """mp_snapshot_cases.canonical_bytes (the stream's default seed): six ticks by `tick` and by the four rounds"""
    import mp_snapshot_cases as c
    from summerset_amd import MpSnapshot
    with exports_of(MpSnapshot) as imgs:
        c.canonical_bytes(dev, oracle, dict(W=W), dict(W=W, how="rounds"), G=G, R=R, S=1, n_ticks=6, every=6)
    return imgs[-1], dict(G=G, R=R, W=W, S=1, n_ticks=6, seed=0x5EED5EED)


def raft_plain(dev, oracle, G=130, R=5, W=8, T=10, seed=43):
    """raft_snapshot_cases.shadow_cluster under ring_schedule: the last replica's image after the last tick"""
    import raft_snapshot_cases as c
    from summerset_amd import RaftSnapshot
    with exports_of(RaftSnapshot) as imgs:
        c.shadow_cluster(dev, oracle, G=G, R=R, W=W, K=8, T=T, make_schedule=c.ring_schedule(R, G, W, seed), arm="many", need=("elected",))
    return imgs[-1], dict(G=G, R=R, W=W, K=8, T=T, seed=seed, arm="many")


def craft_with_queue(dev, oracle, G=130, R=5, W=8, seed=101):
    """raft_snapshot_cases.craft_cluster_form: the last CRaft replica image that carries queued Reconstruct slots (n_rq at byte 40)"""
    import raft_snapshot_cases as c
    from summerset_amd import RaftSnapshot
    with exports_of(RaftSnapshot) as imgs:
        c.craft_cluster_form(dev, oracle, G=G, R=R, W=W, seed=seed)
    return _last(imgs, lambda x: x[15] == 1 and _u64(x, 40) > 0, "a Reconstruct queue"), dict(G=G, R=R, W=W, K=6, seed=seed)


def rsp_replica(dev, oracle, G=130, R=5, W=8, T=12, seed=131):
    """rsp_snapshot_cases.shadow_replicas: the last replica image that carries unpolled executions (n_exec at byte 40)"""
    import rsp_snapshot_cases as c
    from summerset_amd import RSPaxosSnapshot
    with exports_of(RSPaxosSnapshot) as imgs:
        c.shadow_replicas(dev, oracle, G=G, R=R, ft=1, W=W, T=T, seed=seed, rare=False, wrapped=False)
    return _last(imgs, lambda x: _u64(x, 40) > 0, "an unpolled execution list"), dict(G=G, R=R, W=W, ft=1, T=T, seed=seed)


def rsp_store(dev, oracle, G=70, R=3, W=8, L=61, T=14, seed=71):
    """the cluster of rsp_snapshot_cases.shadow_stores (tests/test_zz_rsp_payload_gpu.make_cluster under rsp_scenarios.run) for
    T ticks, every store saved and exported after every tick: the last two-plane image with an aliased vote and a vote stored on
    its own.  (shadow_stores itself runs 44 ticks with a load, an import and a byte-for-byte check of every store after each:
    minutes on the emulator; it has its own tests)"""
    import rsp_scenarios as sc
    import rsp_snapshot_cases as c
    import test_zz_rsp_payload_gpu as tp
    from summerset_amd import PayloadStoreSnapshot
    lay = c.StoreLayout(G, W, 2)

    def both(img):
        _, _, a, _ = lay.parse(img, R // 2 + 1)
        al, av = a[("alias", 1)], a[("avail", 1)]
        return bool((al != 0).any()) and bool(((av & ~al) != 0).any())
    reps, engs = tp.make_cluster(dev, G, R, W, 1, L, False)
    snaps = [PayloadStoreSnapshot.create_like(r.store) for r in reps]
    imgs = []
    sc.run(engs, G, T, seed=seed, loss=0.1, on_tick=lambda t: imgs.extend(r.store.save(s).export() for r, s in zip(reps, snaps)))
    for s in snaps:
        s.close()
    return _last(imgs, both, "an aliased and a stored vote"), dict(G=G, R=R, W=W, ft=1, L=L, T=T, seed=seed)


def craft_store(dev, oracle, G=70, R=3, W=8):
    """rsp_snapshot_cases.craft_shadow_stores (craft_payload_loop's seed 3): the last one-plane store image"""
    import rsp_snapshot_cases as c
    from summerset_amd import PayloadStoreSnapshot
    with exports_of(PayloadStoreSnapshot, on_info=True) as imgs:
        c.craft_shadow_stores(dev, oracle, R, G=G, W=W)
    return imgs[-1], dict(G=G, R=R, W=W, L=200, T=14, seed=3)


KINDS = dict(mp_cluster=mp_cluster, raft_plain=raft_plain, craft_with_queue=craft_with_queue, rsp_replica=rsp_replica, rsp_store=rsp_store,
             craft_store=craft_store)


def digest(img):
    return dict(sha256=hashlib.sha256(img).hexdigest(), bytes=len(img))


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def same_as_recorded(kind, dev, oracle):
    want = golden()["images"][kind]
    img, shape = KINDS[kind](dev, oracle)
    got = dict(digest(img), shape=shape)
    print(kind, got)
    assert got == want, (kind, got, want)
