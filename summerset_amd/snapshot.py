"""The one host-side handle of a device-resident snapshot (`smr_*_snapshot`, csrc/snapshot_common.h).

`MpSnapshot`, `RaftSnapshot`, `RSPaxosSnapshot`, `PayloadStoreSnapshot` and `EPaxosSnapshot` name their C symbols and their info
struct; what a snapshot object does on the host -- make, close, ask its sizes, export, import -- is the same for all five and lives here.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def group_list(groups):
    """a list of groups as the contiguous uint32 host array the `*_groups` calls take (an id that does not fit stays out of
    range, so the library refuses it)"""
    return np.ascontiguousarray(np.asarray(groups, dtype=np.int64).astype(np.uint32))


class DeviceSnapshot:
    _STEM = None       # the C symbols are <stem>_create, _destroy, _info_get, _export, _import
    _INFO = None       # the ctypes struct <stem>_info_get fills

    def __init__(self, like, n_groups=None):
        """room for the worst case of `like`; n_groups (MultiPaxos, Raft, RSPaxos, the payload stores: <stem>_create_groups): for
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
