"""`smr_ep_leader_handle_wire_pre_accept_replies` under the kernel-source emulation (tests/hostsim): the runners of
tests/test_zz_ep_wire_replies_gpu.py with "cpu" as the device -- the shipped kernel source, the shipped C-ABI entry and the
shipped Python mirror, only the device simulated.  Runs without a GPU."""
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_fused_ep_wire_replies_on_the_host(sim, oracle):
    """the fused call against the two calls and the oracle: R = 5, the R = 3 and R = 7 shapes, execution behind it, the emit-stride layout"""
    import test_zz_ep_wire_replies_gpu as t
    with sim.patched():
        assert t.run_fused_ep_wire_replies("cpu", oracle, G=300, R=5, me=2, T=4) > 0
        assert t.run_fused_ep_wire_replies("cpu", oracle, G=600, R=3, me=0, seed=5, T=3) > 0
        assert t.run_fused_ep_wire_replies("cpu", oracle, G=300, R=7, me=6, W=16, seed=6, T=3) > 0
        assert t.run_fused_ep_wire_replies("cpu", oracle, G=300, R=5, me=1, seed=7, T=3, execute=True) > 0
        assert t.run_fused_ep_wire_replies("cpu", oracle, G=300, R=5, me=3, seed=8, T=3, stride=True) > 0


def test_fused_ep_cluster_over_the_wire_on_the_host(sim, oracle):
    import test_zz_ep_wire_replies_gpu as t
    with sim.patched():
        fast, slow = t.run_fused_ep_cluster_over_the_wire("cpu", oracle, T=4)
        assert fast > 0 and slow > 0


def test_fused_ep_wire_replies_edges_on_the_host(sim):
    """a span longer than the LDS stage, a block's located list overflowing, other_cap exceeded, two calls back to back with
    nothing cleared, a partial last block; the refused arguments"""
    import test_zz_ep_wire_replies_gpu as t
    with sim.patched():
        t.run_fused_ep_wire_block_edges("cpu")
        t.run_fused_ep_wire_bad_arguments("cpu")
