"""The device paths of Adversary.search (psg_population_*) and of the shrink (psg_shrink_* with
device_shrink) against the device section of tests/golden/adversary_paths.json, recorded on an
MI355X on the commit named there: every field equal."""
import pytest

from golden import make_adversary_golden as gen

GOLDEN = gen.load()

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(gen.DEVICE_CASES))
def test_device_search_replays_the_golden(name):
    got, want = gen.record_device(name), GOLDEN["device"]["cases"][name]
    for k in sorted(set(got) | set(want)):
        assert got.get(k) == want.get(k), (name, k)
    assert ("shrink_stats" in want) == name.endswith("+dshrink")
