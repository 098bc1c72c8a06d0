"""The one host-side handle of a device-resident snapshot (`smr_*_snapshot`, csrc/snapshot_common.h).

`MpSnapshot`, `RaftSnapshot`, `RSPaxosSnapshot`, `PayloadStoreSnapshot` and `EPaxosSnapshot` name their C symbols and their info
struct; what a snapshot object does on the host -- make, close, ask its sizes, export, import -- is the same for all five and lives here.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, stream_ptr


def group_list(groups):
    """a list of groups as the contiguous uint32 host array the `*_groups` calls take (an id that does not fit stays out of
    range, so the library refuses it)"""
    return np.ascontiguousarray(np.asarray(groups, dtype=np.int64).astype(np.uint32))


class DeviceSnapshot:
    _STEM = None       # the C symbols are <stem>_create, _destroy, _info_get, _export, _import
    _INFO = None       # the ctypes struct <stem>_info_get fills

    def __init__(self, like, n_groups=None):
        """room for the worst case of `like`; n_groups (every engine and the payload stores: <stem>_create_groups): for
        that many of its groups only -- what `save_groups` fills and `load_groups` takes, the image of an n_groups object"""
        self._L = _lib.load()
        h = C.c_void_p()
        if n_groups is None:
            check(self._call("create")(like._h, C.byref(h)))
        else:
            check(self._call("create_groups")(like._h, int(n_groups), C.byref(h)))
        self._h = h

    def _call(self, what):
        return getattr(self._L, "%s_%s" % (self._STEM, what))

    @classmethod
    def create_like(cls, like):
        """room for the worst case of `like`"""
        return cls(like)

    def close(self):
        if getattr(self, "_h", None):
            self._call("destroy")(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def info(self):
        """sizes of what was saved (synchronises)"""
        st = self._INFO()
        check(self._call("info_get")(self._h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_ if n != "reserved"}

    def export(self):
        """the canonical image as bytes"""
        n = self.info()["bytes"]
        buf = (C.c_uint8 * n)()
        got = self._call("export")(self._h, buf, n)
        if got < 0:
            check(int(got))
        return C.string_at(buf, got)

    def import_(self, data):
        """take an exported image (of an object like the one this snapshot was made for)"""
        data = bytes(data)
        check(self._call("import")(self._h, C.cast(C.c_char_p(data), C.c_void_p), len(data)))
        return self


# ---- what an engine object and a cluster of them do with snapshots: the same for every engine, given the C symbol stem
# ("smr_raft": smr_raft_save_groups, smr_raft_cluster_save_groups, ...) and the snapshot class ------------------------------
def _handles(xs):
    return (C.c_void_p * len(xs))(*[x._h for x in xs])


def _sym(stem, what):
    return getattr(_lib.load(), "%s_%s" % (stem, what))


def _glist(groups):
    g = group_list(groups)
    return g, g.ctypes.data_as(C.c_void_p), len(g)


def _paired(what, reps, snaps):
    if len(snaps) != len(reps):
        raise ValueError("%s: %d replicas, %d snapshots" % (what, len(reps), len(snaps)))
    return snaps


def save_state(stem, Snap, obj, snap=None, stream=None):
    snap = Snap(obj) if snap is None else snap
    check(_sym(stem, "save_state")(obj._h, snap._h, stream_ptr(stream)))
    return snap


def load_state(stem, obj, snap, stream=None):
    check(_sym(stem, "load_state")(obj._h, snap._h, stream_ptr(stream)))


def save_groups(stem, Snap, obj, groups, snap=None, stream=None):
    g, p, n = _glist(groups)
    snap = Snap(obj, n) if snap is None else snap
    check(_sym(stem, "save_groups")(obj._h, p, n, snap._h, stream_ptr(stream)))
    return snap


def load_groups(stem, obj, snap, groups, stream=None):
    g, p, n = _glist(groups)
    check(_sym(stem, "load_groups")(obj._h, snap._h, p, n, stream_ptr(stream)))


def reset_groups(stem, obj, groups, stream=None):
    g, p, n = _glist(groups)
    check(_sym(stem, "reset_groups")(obj._h, p, n, stream_ptr(stream)))


def save_cluster_state(stem, Snap, reps, snaps=None, stream=None):
    snaps = _paired("save_cluster_state", reps, [Snap(r) for r in reps] if snaps is None else list(snaps))
    check(_sym(stem, "cluster_save_state")(len(reps), _handles(reps), _handles(snaps), stream_ptr(stream)))
    return snaps


def load_cluster_state(stem, reps, snaps, stream=None):
    _paired("load_cluster_state", reps, snaps)
    check(_sym(stem, "cluster_load_state")(len(reps), _handles(reps), _handles(snaps), stream_ptr(stream)))


def save_cluster_groups(stem, Snap, reps, groups, snaps=None, stream=None):
    g, p, n = _glist(groups)
    snaps = _paired("save_cluster_groups", reps, [Snap(r, n) for r in reps] if snaps is None else list(snaps))
    check(_sym(stem, "cluster_save_groups")(len(reps), _handles(reps), p, n, _handles(snaps), stream_ptr(stream)))
    return snaps


def load_cluster_groups(stem, reps, snaps, groups, stream=None):
    g, p, n = _glist(groups)
    _paired("load_cluster_groups", reps, snaps)
    check(_sym(stem, "cluster_load_groups")(len(reps), _handles(reps), _handles(snaps), p, n, stream_ptr(stream)))


def reset_cluster_groups(stem, reps, groups, stream=None):
    g, p, n = _glist(groups)
    check(_sym(stem, "cluster_reset_groups")(len(reps), _handles(reps), p, n, stream_ptr(stream)))


def move_cluster_groups(stem, Snap, src_reps, src_groups, dst_reps, dst_groups, snaps=None, reset=True):
    snaps = save_cluster_groups(stem, Snap, src_reps, src_groups, snaps)
    load_cluster_groups(stem, dst_reps, snaps, dst_groups)
    if reset:
        reset_cluster_groups(stem, src_reps, src_groups)
    return snaps
