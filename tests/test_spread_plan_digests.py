"""The static plans of layout L2 are the recorded ones (tests/golden/spread_plan_digests.json), and the library's plan builder
gives every exchange the split sizes the Python builder gives it.  The bodies are tests/spread_plan_cases.py; no device: the
engines behind the job objects are the emulator build's (tests/hostsim)."""
import pytest

import spread_plan_cases as c


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


@pytest.mark.parametrize("name", list(c.CASES))
def test_plan_is_the_recorded_one(sim, name):
    with sim.patched():
        c.same_as_recorded(name)


@pytest.mark.parametrize("name", [c.ep_id(x) for x in c.EP_CASES] + [c.rsp_id(x) for x in c.RSP_CASES])
def test_library_plan_has_the_python_plans_split_sizes(sim, name):
    with sim.patched():
        c.library_splits_agree(name)


def test_every_case_is_recorded():
    assert sorted(c.golden()["cases"]) == sorted(c.CASES)
