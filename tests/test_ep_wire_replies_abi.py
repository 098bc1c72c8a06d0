"""`smr_ep_leader_handle_wire_pre_accept_replies`: the null-argument errors come back without a device (a null replica and null
outputs are refused before anything is dereferenced or launched)."""
import pytest


def test_null_arguments_are_refused_without_a_device(engine_lib):
    from summerset_amd import _lib
    from summerset_amd._lib import SummersetError, check
    fn = engine_lib.smr_ep_leader_handle_wire_pre_accept_replies
    # (replica, buf, buf_len, conn_off, conn_len, n_conn, col, order, exploded, decision, d_seq, d_deps, others, other_cap, counts, consumed,
    #  status, stream); 0x1000: a non-null pointer that is never dereferenced -- every call below fails on an argument in front
    P = 0x1000
    null_replica = (None, P, 16, P, None, 4, P, None, None, P, P, P, P, 4, P, P, P, None)
    with pytest.raises(SummersetError) as e:
        check(fn(*null_replica))
    assert e.value.code == _lib.SMR_ERR_ARG and "epaxos wire replies: null argument" in e.value.msg
    for i in (3, 6, 9, 10, 11, 14, 15, 16):                        # conn_off, col, decision, d_seq, d_deps, counts, consumed, status
        args = list(null_replica)
        args[i] = None
        with pytest.raises(SummersetError) as e:
            check(fn(*args))
        assert e.value.code == _lib.SMR_ERR_ARG and "null argument" in e.value.msg, i
    with pytest.raises(SummersetError) as e:                       # (all nulls)
        check(fn(None, None, 0, None, None, 0, None, None, None, None, None, None, None, 0, None, None, None, None))
    assert e.value.code == _lib.SMR_ERR_ARG
